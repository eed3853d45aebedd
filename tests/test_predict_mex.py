"""tci_mex('predict', ...) through the stand-in MATLAB API: its argument checks (CPU; they come before
the handle is touched) and, on the GPU, its bands against Likelihood.predict bit for bit, with
MATLAB's conventions: X is P x S x n column-major, cells are 1-based, outputs are N_max x nq x n."""
import ctypes as C

import numpy as np
import pytest

from mexharness import MxPtr
from test_mex_gateway import data_struct, expect, mex  # noqa: F401  (mex: the module's gateway fixture)

PROBS = np.array([0.0, 0.025, 0.5, 0.975, 1.0])


def nd_double(mex, a):
    """A MATLAB double array of any rank (mexharness.double builds matrices only)."""
    a = np.asarray(a, np.float64)
    f = mex.L.mxCreateNumericArray
    f.restype, f.argtypes = C.c_void_p, [C.c_size_t, C.POINTER(C.c_size_t), C.c_int, C.c_int]
    dims = (C.c_size_t * a.ndim)(*a.shape)
    p = f(a.ndim, dims, 6, 0)   # mxDOUBLE_CLASS, mxREAL
    if a.size:
        fa = np.asfortranarray(a)
        C.memmove(mex.L.mxGetData(p), fa.ctypes.data, 8 * a.size)
    return MxPtr(mex, p)


def test_predict_arguments_are_checked(mex):
    fake = MxPtr(mex, mex.handle(12345))
    X = nd_double(mex, np.zeros((130, 4, 2)))
    cells12 = np.array([1.0, 2.0])
    try:
        expect("tci:handle", mex.call, "predict", fake, cells12, X, PROBS, "raw", nlhs=2)   # only the handle is bad
        expect("tci:handle", mex.call, "predict", fake, cells12, X, PROBS, nlhs=2)          # the grid defaults to raw
        expect("tci:arg", mex.call, "predict", fake, cells12, X)                            # too few arguments
        expect("tci:arg", mex.call, "predict", fake, cells12, X, PROBS, "raw", 1.0)         # too many
        expect("tci:arg", mex.call, "predict", fake, np.array([1.0, 2.0, 3.0]), X, PROBS)   # n differs from X's pages
        expect("tci:arg", mex.call, "predict", fake, np.zeros(0), X, PROBS)
        expect("tci:arg", mex.call, "predict", fake, np.array([0.0, 1.0]), X, PROBS)        # cells are 1-based
        expect("tci:arg", mex.call, "predict", fake, np.array([1.5, 1.0]), X, PROBS)
        expect("tci:arg", mex.call, "predict", fake, cells12, X, np.zeros(0))               # probs: 1 to 16
        expect("tci:arg", mex.call, "predict", fake, cells12, X, np.full(17, 0.5))
        expect("tci:arg", mex.call, "predict", fake, cells12, X, np.array([0.5, 1.5]))
        expect("tci:arg", mex.call, "predict", fake, cells12, X, np.array([np.nan]))
        expect("tci:arg", mex.call, "predict", fake, cells12, X, PROBS, "uniform")
        expect("tci:arg", mex.call, "predict", fake, cells12, X, PROBS, 1.0)                # the grid is a string
        lg = MxPtr(mex, mex.logical([True, False]))
        expect("tci:arg", mex.call, "predict", fake, cells12, lg, PROBS)                    # X must be double
        lg.free()
        for shape in ((8, 4, 2), (130, 4097, 2), (130, 4, 2, 2)):
            bad = nd_double(mex, np.zeros(shape))
            expect("tci:arg", mex.call, "predict", fake, cells12, bad, PROBS)
            bad.free()
        one = nd_double(mex, np.zeros((130, 4)))                                            # P x S x 1 == P x S
        expect("tci:handle", mex.call, "predict", fake, np.array([1.0]), one, PROBS)
        expect("tci:arg", mex.call, "predict", fake, cells12, one, PROBS)
        one.free()
    finally:
        X.free()
        fake.free()


@pytest.mark.gpu
def test_predict_equals_the_binding_bitwise(mex, cells):
    from transcriptioncycleinference_amd import Likelihood
    from transcriptioncycleinference_amd.data import draw_x0

    d = data_struct(mex, cells, range(cells.n_cells))
    h = mex.call("create", d, "P2P-MS2v5-LacZ-PP7v4", 0.0)[0]
    d.free()
    gw = MxPtr(mex, mex.handle(int(h[0, 0])))
    rng = np.random.default_rng(21)
    cid = np.array([298, 0, 150, 42], np.int32)
    S, P = 37, 7 + int(cells.lengths.max())
    theta = np.zeros((len(cid), S, P))
    for k, c in enumerate(cid):
        for s in range(S):
            r = draw_x0(rng, int(cells.lengths[c]))
            theta[k, s, :len(r)] = r
    X = nd_double(mex, np.transpose(theta, (2, 1, 0)))     # P x S x n
    try:
        with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
            for grid in ("raw", "interp"):
                ms2, pp7 = mex.call("predict", gw, (cid + 1).astype(np.float64), X, PROBS, grid, nlhs=2)
                wm, wp = lk.predict(theta, cid, probs=PROBS, grid=grid)
                nmax = int(cells.lengths[cid].max())
                assert ms2.shape == (nmax, len(PROBS), len(cid)) == pp7.shape
                assert np.transpose(ms2, (2, 1, 0)).tobytes() == wm.tobytes()   # N_max x nq x n == [cell][q][N_max]
                assert np.transpose(pp7, (2, 1, 0)).tobytes() == wp.tobytes()
            only = mex.call("predict", gw, (cid + 1).astype(np.float64), X, PROBS, nlhs=1)[0]
            assert np.array_equal(np.transpose(only, (2, 1, 0)), lk.predict(theta, cid, probs=PROBS)[0], equal_nan=True)
        expect("tci:call", mex.call, "predict", gw, np.array([300.0, 1.0, 2.0, 3.0]), X, PROBS)   # cell 300 of 299
    finally:
        X.free()
        mex.call("destroy", gw, nlhs=0)
        gw.free()
