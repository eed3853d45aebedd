"""tci_mex('fitcheck', ...) through the stand-in MATLAB API: its argument checks (CPU; they come before the handle is
touched) and, on the GPU, its outputs against Likelihood.fitcheck bit for bit, with MATLAB's conventions: X is
P x S x n and s2 S x n column-major, cells are 1-based, the pointwise arrays are N_max x 2 x n."""
import numpy as np
import pytest

from mexharness import MxPtr
from test_mex_gateway import data_struct, expect, mex  # noqa: F401  (mex: the module's gateway fixture)
from test_predict_mex import nd_double

LEVELS = np.array([0.5, 0.8, 0.95])


def test_fitcheck_arguments_are_checked(mex):
    fake = MxPtr(mex, mex.handle(12345))
    X = nd_double(mex, np.zeros((130, 4, 2)))
    cells12 = np.array([1.0, 2.0])
    s2 = np.ones((4, 2))
    try:
        expect("tci:handle", mex.call, "fitcheck", fake, cells12, X, s2, LEVELS, nlhs=2)   # only the handle is bad
        expect("tci:handle", mex.call, "fitcheck", fake, cells12, X, s2, nlhs=2)           # the levels default
        expect("tci:arg", mex.call, "fitcheck", fake, cells12, X)                          # too few arguments
        expect("tci:arg", mex.call, "fitcheck", fake, cells12, X, s2, LEVELS, 1.0)         # too many
        expect("tci:arg", mex.call, "fitcheck", fake, np.array([1.0, 2.0, 3.0]), X, s2)    # n differs from X's pages
        expect("tci:arg", mex.call, "fitcheck", fake, np.zeros(0), X, s2)
        expect("tci:arg", mex.call, "fitcheck", fake, np.array([0.0, 1.0]), X, s2)         # cells are 1-based
        expect("tci:arg", mex.call, "fitcheck", fake, np.array([1.5, 1.0]), X, s2)
        expect("tci:arg", mex.call, "fitcheck", fake, cells12, X, np.ones((4, 3)))         # s2 is S x n
        expect("tci:arg", mex.call, "fitcheck", fake, cells12, X, np.ones((2, 4)))
        for bad in (0.0, -1.0, np.nan, np.inf):
            b = s2.copy()
            b[3, 1] = bad
            e = expect("tci:arg", mex.call, "fitcheck", fake, cells12, X, b)
            assert "s2(8)" in e.msg                                                        # column-major, 1-based
        expect("tci:arg", mex.call, "fitcheck", fake, cells12, X, s2, np.zeros(0))         # levels: 1 to 8
        expect("tci:arg", mex.call, "fitcheck", fake, cells12, X, s2, np.full(9, 0.5))
        for bad in (0.0, 1.0, 1.5, np.nan):
            expect("tci:arg", mex.call, "fitcheck", fake, cells12, X, s2, np.array([0.5, bad]))
        lg = MxPtr(mex, mex.logical([True, False]))
        expect("tci:arg", mex.call, "fitcheck", fake, cells12, lg, s2)                     # X must be double
        lg.free()
        for shape in ((8, 4, 2), (130, 4, 2, 2)):
            bad = nd_double(mex, np.zeros(shape))
            expect("tci:arg", mex.call, "fitcheck", fake, cells12, bad, s2)
            bad.free()
        big = nd_double(mex, np.zeros((9, 4097, 2)))
        expect("tci:arg", mex.call, "fitcheck", fake, cells12, big, np.ones((4097, 2)))
        big.free()
        one = nd_double(mex, np.zeros((130, 4)))                                           # P x S x 1 == P x S
        expect("tci:handle", mex.call, "fitcheck", fake, np.array([1.0]), one, np.ones((4, 1)))
        expect("tci:arg", mex.call, "fitcheck", fake, cells12, one, s2)
        one.free()
    finally:
        X.free()
        fake.free()


@pytest.mark.gpu
def test_fitcheck_equals_the_binding_bitwise(mex, cells):
    from transcriptioncycleinference_amd import Likelihood
    from transcriptioncycleinference_amd.data import draw_x0

    d = data_struct(mex, cells, range(cells.n_cells))
    h = mex.call("create", d, "P2P-MS2v5-LacZ-PP7v4", 0.0)[0]
    d.free()
    gw = MxPtr(mex, mex.handle(int(h[0, 0])))
    rng = np.random.default_rng(22)
    cid = np.array([298, 0, 150, 42], np.int32)
    S, P = 70, 7 + int(cells.lengths.max())
    theta = np.zeros((len(cid), S, P))
    for k, c in enumerate(cid):
        for s in range(S):
            r = draw_x0(rng, int(cells.lengths[c]))
            theta[k, s, :len(r)] = r
    s2 = rng.uniform(5.0, 20.0, (len(cid), S))
    X = nd_double(mex, np.transpose(theta, (2, 1, 0)))     # P x S x n
    one = (cid + 1).astype(np.float64)
    try:
        with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
            for levels in (LEVELS, None):
                args = (s2.T,) if levels is None else (s2.T, levels)
                pt, cell = mex.call("fitcheck", gw, one, X, *args, nlhs=2)
                want = lk.fitcheck(theta, s2, cid, **({} if levels is None else {"levels": levels}))
                nmax = int(cells.lengths[cid].max())
                assert list(pt) == ["lppd", "p_waic", "pit", "resid", "zbar", "z2"]
                for f, w in zip(pt, ("lppd_i", "p_waic_i", "pit", "resid", "zbar", "z2")):
                    assert pt[f].shape == (nmax, 2, len(cid))
                    assert np.transpose(pt[f], (2, 1, 0)).tobytes() == getattr(want, w).tobytes(), f
                for f in ("lppd", "p_waic", "elpd_waic", "chi2"):
                    assert cell[f].shape == (1, len(cid)) and cell[f][0].tobytes() == getattr(want, f).tobytes(), f
                assert cell["n_obs"][0].tolist() == want.n_obs.tolist()
                assert cell["coverage"].shape == (len(want.levels), len(cid))
                assert cell["coverage"].T.tobytes() == want.coverage.tobytes()     # n_levels x n == [cell][level]
                assert cell["dw"].shape == (2, len(cid)) and cell["dw"].T.tobytes() == want.dw.tobytes()
                assert cell["levels"][0].tolist() == want.levels.tolist() and cell["kernel_ms"][0, 0] > 0
            only = mex.call("fitcheck", gw, one, X, s2.T, nlhs=1)[0]
            assert np.array_equal(np.transpose(only["pit"], (2, 1, 0)), want.pit, equal_nan=True)
        expect("tci:call", mex.call, "fitcheck", gw, np.array([300.0, 1.0, 2.0, 3.0]), X, s2.T)   # cell 300 of 299
    finally:
        X.free()
        mex.call("destroy", gw, nlhs=0)
        gw.free()
