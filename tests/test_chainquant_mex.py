"""tci_mex('chainquant', ...) through the stand-in MATLAB API: argument checks (CPU; they come before the handle
is touched) and, on the GPU, bitwise equality with the Python binding, in MATLAB's conventions: chain is
P x n x rows, q is P x nq x n."""
import numpy as np
import pytest

import chaincov_oracle as CO
from mexharness import MxPtr
from test_mex_gateway import data_struct, expect, mex  # noqa: F401  (mex: the gateway fixture)
from test_predict_mex import nd_double


def test_chainquant_arguments_are_checked(mex):
    fake = MxPtr(mex, mex.handle(12345))
    X = nd_double(mex, np.zeros((9, 2, 30)))
    none = np.zeros((0, 0))
    pr = np.array([0.025, 0.5, 0.975])
    try:
        expect("tci:handle", mex.call, "chainquant", fake, X, np.array([9.0, 8.0]), pr)   # only the handle is bad
        expect("tci:handle", mex.call, "chainquant", fake, X, none, pr)                   # [] npar
        expect("tci:arg", mex.call, "chainquant", fake, X, none)                          # too few arguments
        expect("tci:arg", mex.call, "chainquant", fake, X, none, pr, 0.0)                 # too many
        expect("tci:arg", mex.call, "chainquant", fake, X, np.array([9.0]), pr)           # one npar per chain
        expect("tci:arg", mex.call, "chainquant", fake, X, np.array([10.0, 1.0]), pr)     # npar <= P
        expect("tci:arg", mex.call, "chainquant", fake, X, np.array([1.5, 1.0]), pr)
        expect("tci:arg", mex.call, "chainquant", fake, X, none, none)                    # no probs
        expect("tci:arg", mex.call, "chainquant", fake, X, none, np.linspace(0, 1, 17))   # more than 16
        expect("tci:arg", mex.call, "chainquant", fake, X, none, np.array([0.5, -0.1]))
        expect("tci:arg", mex.call, "chainquant", fake, X, none, np.array([np.nan]))
        lg = MxPtr(mex, mex.logical([True, False]))
        expect("tci:arg", mex.call, "chainquant", fake, lg, none, pr)                     # chain must be double
        lg.free()
        bad = nd_double(mex, np.zeros((9, 2, 30, 2)))
        expect("tci:arg", mex.call, "chainquant", fake, bad, none, pr)
        bad.free()
    finally:
        X.free()
        fake.free()


@pytest.mark.gpu
def test_chainquant_equals_the_binding_bitwise(mex, cells):
    from transcriptioncycleinference_amd import Likelihood

    d = data_struct(mex, cells, range(cells.n_cells))
    h = mex.call("create", d, "P2P-MS2v5-LacZ-PP7v4", 0.0)[0]
    d.free()
    gw = MxPtr(mex, mex.handle(int(h[0, 0])))
    rows, n, P = 257, 3, 37
    npar = np.array([37, 16, 33], np.int32)
    probs = np.array([0.0, 0.025, 0.5, 0.975, 1.0])
    chain = CO.walk_chain(21, rows, n, P, npar)
    X = nd_double(mex, np.transpose(chain, (2, 1, 0)))       # P x n x rows
    try:
        with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
            got = mex.call("chainquant", gw, X, npar.astype(np.float64), probs)[0]
            want = lk.chainquant(chain, None, npar, probs)
            assert got["q"].shape == (P, 5, n) and got["n_rows"][0, 0] == rows
            assert np.ascontiguousarray(np.transpose(got["q"], (2, 1, 0))).tobytes() == want.q.tobytes()
            bare = mex.call("chainquant", gw, X, np.zeros((0, 0)), probs)[0]
            assert np.ascontiguousarray(np.transpose(bare["q"], (2, 1, 0))).tobytes() == \
                lk.chainquant(chain, probs=probs).q.tobytes()
    finally:
        X.free()
        mex.call("destroy", gw, nlhs=0)
        gw.free()
