"""tci_mex('chaincov', ...) through the stand-in MATLAB API: argument checks (CPU; they come before the handle
is touched) and, on the GPU, bitwise equality with the Python binding, in MATLAB's conventions: chain is
P x n x rows, mean P x n, cov and corr P x P x n."""
import numpy as np
import pytest

import chaincov_oracle as O
from mexharness import MxPtr
from test_mex_gateway import data_struct, expect, mex  # noqa: F401  (mex: the gateway fixture)
from test_predict_mex import nd_double


def test_chaincov_arguments_are_checked(mex):
    fake = MxPtr(mex, mex.handle(12345))
    X = nd_double(mex, np.zeros((9, 2, 30)))
    none = np.zeros((0, 0))
    try:
        expect("tci:handle", mex.call, "chaincov", fake, X, np.array([9.0, 8.0]))       # only the handle is bad
        expect("tci:handle", mex.call, "chaincov", fake, X, none)                       # [] npar
        expect("tci:arg", mex.call, "chaincov", fake, X)                                # too few arguments
        expect("tci:arg", mex.call, "chaincov", fake, X, none, 0.0)                     # too many
        expect("tci:arg", mex.call, "chaincov", fake, X, np.array([9.0]))               # one npar per chain
        expect("tci:arg", mex.call, "chaincov", fake, X, np.array([10.0, 1.0]))         # npar <= P
        expect("tci:arg", mex.call, "chaincov", fake, X, np.array([1.5, 1.0]))
        expect("tci:arg", mex.call, "chaincov", fake, X, np.array([-1.0, 1.0]))
        lg = MxPtr(mex, mex.logical([True, False]))
        expect("tci:arg", mex.call, "chaincov", fake, lg, none)                         # chain must be double
        lg.free()
        bad = nd_double(mex, np.zeros((9, 2, 30, 2)))
        expect("tci:arg", mex.call, "chaincov", fake, bad, none)
        bad.free()
    finally:
        X.free()
        fake.free()


@pytest.mark.gpu
def test_chaincov_equals_the_binding_bitwise(mex, cells):
    from transcriptioncycleinference_amd import Likelihood

    d = data_struct(mex, cells, range(cells.n_cells))
    h = mex.call("create", d, "P2P-MS2v5-LacZ-PP7v4", 0.0)[0]
    d.free()
    gw = MxPtr(mex, mex.handle(int(h[0, 0])))
    rows, n, P = 257, 3, 37
    npar = np.array([37, 16, 33], np.int32)
    chain = O.walk_chain(21, rows, n, P, npar)
    X = nd_double(mex, np.transpose(chain, (2, 1, 0)))       # P x n x rows
    try:
        with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
            got = mex.call("chaincov", gw, X, npar.astype(np.float64))[0]
            want = lk.chaincov(chain, npar)
            assert got["mean"].shape == (P, n) and got["cov"].shape == (P, P, n) == got["corr"].shape
            assert np.ascontiguousarray(got["mean"].T).tobytes() == want.mean.tobytes()
            for k in ("cov", "corr"):
                assert np.ascontiguousarray(np.transpose(got[k], (2, 1, 0))).tobytes() == getattr(want, k).tobytes(), k
            assert got["n_rows"][0, 0] == rows and got["kernel_ms"][0, 0] > 0
            bare = mex.call("chaincov", gw, X, np.zeros((0, 0)))[0]
            assert np.ascontiguousarray(np.transpose(bare["cov"], (2, 1, 0))).tobytes() == lk.chaincov(chain).cov.tobytes()
            one = nd_double(mex, np.zeros((P, n, 1)))        # fewer than 2 rows: the library refuses
            expect("tci:call", mex.call, "chaincov", gw, one, np.zeros((0, 0)))
            one.free()
    finally:
        X.free()
        mex.call("destroy", gw, nlhs=0)
        gw.free()
