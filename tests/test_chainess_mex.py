"""tci_mex('chainess', ...) through the stand-in MATLAB API: argument checks (CPU; they come before the handle is
touched) and, on the GPU, bitwise equality with the Python binding, in MATLAB's conventions: chain is P x n x rows,
the outputs are P x n_groups (the windows as doubles), group is 1-based (0 = in no group)."""
import numpy as np
import pytest

import chainess_oracle as O
from mexharness import MxPtr
from test_mex_gateway import data_struct, expect, mex  # noqa: F401  (mex: the gateway fixture)
from test_predict_mex import nd_double


def test_chainess_arguments_are_checked(mex):
    fake = MxPtr(mex, mex.handle(12345))
    X = nd_double(mex, np.zeros((9, 2, 30)))
    none = np.zeros((0, 0))
    try:
        expect("tci:handle", mex.call, "chainess", fake, X, np.array([9.0, 9.0]), np.array([1.0, 1.0]))  # only the handle
        expect("tci:handle", mex.call, "chainess", fake, X, none, none, 5.0)              # [] npar, [] group, a cap
        expect("tci:arg", mex.call, "chainess", fake, X, none)                            # too few arguments
        expect("tci:arg", mex.call, "chainess", fake, X, none, none, 0.0, 0.0)            # too many
        expect("tci:arg", mex.call, "chainess", fake, X, none, none, -1.0)                # max_lag >= 0
        expect("tci:arg", mex.call, "chainess", fake, X, none, none, 1.5)
        expect("tci:arg", mex.call, "chainess", fake, X, np.array([10.0, 1.0]), none)     # npar <= P
        expect("tci:arg", mex.call, "chainess", fake, X, none, np.array([1.0, 3.0]))      # group <= n
        expect("tci:arg", mex.call, "chainess", fake, X, none, np.array([0.0, 0.0]))      # no group at all
    finally:
        X.free()
        fake.free()


@pytest.mark.gpu
def test_chainess_equals_the_binding_bitwise(mex, cells):
    from transcriptioncycleinference_amd import Likelihood

    d = data_struct(mex, cells, range(cells.n_cells))
    h = mex.call("create", d, "P2P-MS2v5-LacZ-PP7v4", 0.0)[0]
    d.free()
    gw = MxPtr(mex, mex.handle(int(h[0, 0])))
    rows, n, P = 257, 6, 37
    group = np.array([1, 0, 1, -1, 0, 1], np.int32)
    npar = np.array([16, 37, 16, 33, 37, 16], np.int32)
    chain, _ = O.ar1_chains(21, rows, n, P, npar)
    X = nd_double(mex, np.transpose(chain, (2, 1, 0)))       # P x n x rows
    try:
        with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
            for lag in (None, 65.0):
                extra = () if lag is None else (lag,)
                got = mex.call("chainess", gw, X, npar.astype(np.float64), (group + 1).astype(np.float64), *extra)[0]
                want = lk.chainess(chain, None, npar, group, max_lag=int(lag or 0))
                assert got["n_rows"][0, 0] == rows
                for k in O.OUTPUTS:
                    assert got[k].shape == (P, 2)
                    assert np.ascontiguousarray(got[k].T).tobytes() == getattr(want, k).tobytes(), k
                for k in O.WINDOWS:
                    assert np.array_equal(got[k].T, getattr(want, k).astype(np.float64)), k
            bare = mex.call("chainess", gw, X, np.zeros((0, 0)), np.zeros((0, 0)))[0]
            assert bare["ess"].shape == (P, 1)
            assert np.ascontiguousarray(bare["ess"].T).tobytes() == lk.chainess(chain).ess.tobytes()
    finally:
        X.free()
        mex.call("destroy", gw, nlhs=0)
        gw.free()
