"""tci_mex('chaindens', ...) through the stand-in MATLAB API: argument and option checks (CPU; they come before
the handle is touched) and, on the GPU, bitwise equality with the Python binding, in MATLAB's conventions: chain
is P x n x rows, s2chain n x rows, dens and grid P x n_grid x n, counts P x n_bins x n (as doubles)."""
import numpy as np
import pytest

import chaincov_oracle as CO
from mexharness import MxPtr
from test_mex_gateway import data_struct, expect, mex  # noqa: F401  (mex: the gateway fixture)
from test_predict_mex import nd_double


def opts(mex, **kv):  # noqa: F811
    return MxPtr(mex, mex.struct([kv], list(kv)))


def test_chaindens_arguments_are_checked(mex):  # noqa: F811
    fake = MxPtr(mex, mex.handle(12345))
    X = nd_double(mex, np.zeros((9, 2, 30)))
    none = np.zeros((0, 0))
    s2 = np.ones((2, 30))
    made = [fake, X]
    try:
        expect("tci:handle", mex.call, "chaindens", fake, X, s2, np.array([9.0, 8.0]))   # only the handle is bad
        expect("tci:handle", mex.call, "chaindens", fake, X, none, none)                 # [] s2chain, [] npar
        expect("tci:handle", mex.call, "chaindens", fake, X, none, none, none)           # [] options
        good = opts(mex, n_grid=50.0, n_bins=7.0, bw_scale=0.5)
        made.append(good)
        expect("tci:handle", mex.call, "chaindens", fake, X, s2, none, good)
        expect("tci:arg", mex.call, "chaindens", fake, X, none)                          # too few arguments
        expect("tci:arg", mex.call, "chaindens", fake, X, none, none, none, 0.0)         # too many
        expect("tci:arg", mex.call, "chaindens", fake, X, none, np.array([9.0]))         # one npar per chain
        expect("tci:arg", mex.call, "chaindens", fake, X, none, np.array([10.0, 1.0]))   # npar <= P
        expect("tci:arg", mex.call, "chaindens", fake, X, none, np.array([1.5, 1.0]))
        expect("tci:arg", mex.call, "chaindens", fake, X, np.ones((30, 2)), none)        # s2chain is n x rows
        expect("tci:arg", mex.call, "chaindens", fake, X, np.ones((2, 29)), none)
        lg = MxPtr(mex, mex.logical([True, False]))
        made.append(lg)
        expect("tci:arg", mex.call, "chaindens", fake, lg, none, none)                   # chain must be double
        for a in (np.zeros((9, 2, 30, 2)), np.zeros((9, 2, 1))):                         # rank, fewer than 2 rows
            bad = nd_double(mex, a)
            made.append(bad)
            expect("tci:arg", mex.call, "chaindens", fake, bad, none, none)
        for kv in (dict(n_grid=1.0), dict(n_grid=257.0), dict(n_grid=2.5), dict(n_bins=0.0), dict(n_bins=257.0),
                   dict(bw_scale=0.0), dict(bw_scale=-1.0), dict(bw_scale=np.nan), dict(bw_scale=np.inf),
                   dict(n_grid=np.array([3.0, 4.0])), dict(n_grid="many"), dict(probs=0.5)):
            o = opts(mex, **kv)
            made.append(o)
            expect("tci:opts", mex.call, "chaindens", fake, X, none, none, o)
        expect("tci:opts", mex.call, "chaindens", fake, X, none, none, 3.0)              # options must be a struct
    finally:
        for m in made:
            m.free()


@pytest.mark.gpu
def test_chaindens_equals_the_binding_bitwise(mex, cells):  # noqa: F811
    from transcriptioncycleinference_amd import Likelihood

    d = data_struct(mex, cells, range(cells.n_cells))
    h = mex.call("create", d, "P2P-MS2v5-LacZ-PP7v4", 0.0)[0]
    d.free()
    gw = MxPtr(mex, mex.handle(int(h[0, 0])))
    rows, n, P = 257, 3, 37
    npar = np.array([37, 16, 33], np.int32)
    chain = CO.walk_chain(21, rows, n, P, npar)
    s2 = np.random.default_rng(5).gamma(3.0, 2.0, (rows, n))
    X = nd_double(mex, np.transpose(chain, (2, 1, 0)))       # P x n x rows
    o = opts(mex, n_grid=33.0, n_bins=7.0, bw_scale=0.5)
    t3 = lambda a: np.ascontiguousarray(np.transpose(a, (2, 1, 0)))  # noqa: E731  P x k x n -> [n][k][P]
    try:
        with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
            got = mex.call("chaindens", gw, X, s2.T, npar.astype(np.float64), o)[0]
            want = lk.chaindens(chain, s2, npar, n_grid=33, n_bins=7, bw_scale=0.5)
            assert got["dens"].shape == (P, 33, n) and got["counts"].shape == (P, 7, n) and got["n_rows"][0, 0] == rows
            assert got["range"].shape == (P, 2, n) and got["bw"].shape == (P, n) and got["s2_dens"].shape == (33, n)
            assert t3(got["dens"]).tobytes() == want.dens.tobytes()
            assert t3(got["range"]).tobytes() == want.range.tobytes()
            assert np.ascontiguousarray(got["bw"].T).tobytes() == want.bw.tobytes()
            assert np.array_equal(t3(got["counts"]), want.counts.astype(np.float64))
            real = ~np.isnan(want.grid())
            assert np.array_equal(np.isnan(t3(got["grid"])), ~real)
            assert t3(got["grid"])[real].tobytes() == want.grid()[real].tobytes()
            assert np.ascontiguousarray(got["s2_dens"].T).tobytes() == want.s2_dens.tobytes()
            assert np.ascontiguousarray(got["s2_range"].T).tobytes() == want.s2_range.tobytes()
            assert np.ascontiguousarray(got["s2_grid"].T).tobytes() == want.s2_grid().tobytes()
            assert np.ascontiguousarray(got["s2_bw"]).tobytes() == want.s2_bw.tobytes()
            assert np.array_equal(got["s2_counts"].T, want.s2_counts.astype(np.float64))
            bare = mex.call("chaindens", gw, X, np.zeros((0, 0)), np.zeros((0, 0)))[0]    # the defaults, no s2
            dflt = lk.chaindens(chain)
            assert t3(bare["dens"]).tobytes() == dflt.dens.tobytes() and bare["counts"].shape == (P, 20, n)
            assert np.all(np.isnan(bare["s2_dens"])) and np.all(bare["s2_counts"] == -1)
    finally:
        X.free()
        o.free()
        mex.call("destroy", gw, nlhs=0)
        gw.free()
