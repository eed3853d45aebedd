"""tci_mex('chainlp', ...) and the 'logpost' option of tci_mex('dram', ...) through the stand-in MATLAB API: argument
checks (CPU; they come before the handle is touched) and, on the GPU, bitwise equality with the Python binding, in
MATLAB's conventions: chain is P x n x rows, s2chain n x rows, the traces n x rows, the per-chain scalars 1 x n,
theta_best and theta_mean P x n, cells and best_row 1-based (best_row 0 = none)."""
import numpy as np
import pytest

import chainlp_oracle as O
from mexharness import MxPtr
from test_mex_gateway import _dram_args, _opts, data_struct, expect, mex  # noqa: F401  (mex: the gateway fixture)
from test_predict_mex import nd_double

TRACES = ("ss", "pri", "dev", "lp")


def test_chainlp_arguments_are_checked(mex):
    fake = MxPtr(mex, mex.handle(12345))
    X = nd_double(mex, np.zeros((30, 2, 9)))            # P x n x rows
    cells, s2, M = np.array([1.0, 2.0]), np.ones((2, 9)), np.ones((30, 2))
    try:
        expect("tci:handle", mex.call, "chainlp", fake, cells, X, s2, M, M)          # well-formed: only the handle
        expect("tci:arg", mex.call, "chainlp", fake, cells, X, s2, M)                # too few arguments
        expect("tci:arg", mex.call, "chainlp", fake, cells, X, s2, M, M, 0.0)        # too many
        expect("tci:arg", mex.call, "chainlp", fake, np.array([1.0]), X, s2, M, M)   # one cell per chain
        e = expect("tci:arg", mex.call, "chainlp", fake, np.array([1.0, 0.0]), X, s2, M, M)   # cells are 1-based
        assert "cells(2)" in e.msg
        expect("tci:arg", mex.call, "chainlp", fake, cells + 0.5, X, s2, M, M)
        expect("tci:arg", mex.call, "chainlp", fake, cells, X, np.ones((9, 2)), M, M)     # s2chain is n x rows
        expect("tci:arg", mex.call, "chainlp", fake, cells, X, np.ones((2, 8)), M, M)
        assert "MU" in expect("tci:arg", mex.call, "chainlp", fake, cells, X, s2, M[:29], M).msg
        assert "SIG" in expect("tci:arg", mex.call, "chainlp", fake, cells, X, s2, M, M[:, :1]).msg
    finally:
        X.free()
        fake.free()


def test_dram_logpost_option_is_checked(mex, cells):
    fake = MxPtr(mex, mex.handle(12345))
    _, a = _dram_args(mex, cells, [0, 1, 2])
    for kv, word in (({"logpost": [1.0, 0.0]}, "logpost"), ({"logpost": "yes"}, "logpost"),
                     ({"logpost": 1.0, "thin": 0.0}, "thin"),
                     ({"logpost": True, "nsimu": 50.0, "burnintime": 10.0, "stats_from": 51.0}, "stats_from")):
        o = _opts(mex, **kv)
        e = expect("tci:opts", mex.call, "dram", fake, *a, o)
        assert word in e.msg, (kv, e.msg)
        o.free()
    o = _opts(mex, logpost=True, nsimu=50.0, burnintime=10.0)
    expect("tci:handle", mex.call, "dram", fake, *a, o)
    o.free()
    fake.free()


def same_struct(got, want, n, P, rows):
    """The gateway's struct against a ChainLp, bit for bit."""
    assert got["n_rows"][0, 0] == rows == want.n_rows
    for f in TRACES:
        assert got[f].shape == (n, rows)
        assert np.ascontiguousarray(got[f].T).tobytes() == getattr(want, f).tobytes(), f
    for f in O.SCALARS:
        assert got[f].shape == (1, n) and got[f][0].tobytes() == getattr(want, f).tobytes(), f
    assert np.array_equal(got["best_row"][0], want.best_row.astype(np.float64) + 1.0)
    for f in ("theta_best", "theta_mean"):
        assert got[f].shape == (P, n)
        assert np.ascontiguousarray(got[f].T).tobytes() == getattr(want, f).tobytes(), f


@pytest.mark.gpu
def test_chainlp_equals_the_binding_bitwise(mex, cells):
    from transcriptioncycleinference_amd import Likelihood, _lib
    from transcriptioncycleinference_amd.data import draw_x0

    d = data_struct(mex, cells, range(cells.n_cells))
    h = mex.call("create", d, "P2P-MS2v5-LacZ-PP7v4", 0.0)[0]
    d.free()
    gw = MxPtr(mex, mex.handle(int(h[0, 0])))
    order = np.argsort(cells.lengths, kind="stable")
    cid = np.array([order[0], order[-1], order[len(order) // 2]], np.int32)
    rows, n = 257, 3
    Pc = 7 + cells.lengths[cid]
    P = int(Pc.max())
    rng = np.random.default_rng(77)
    chain = np.full((rows, n, P), np.nan)
    mu, sig = np.zeros((n, P)), np.full((n, P), np.inf)
    for c in range(n):
        for t in range(rows):
            chain[t, c, :Pc[c]] = draw_x0(rng, int(cells.lengths[cid[c]]))
        sig[c, 7:Pc[c]] = 50.0
    s2 = rng.uniform(50.0, 150.0, (rows, n))
    chain[100, 1, 3] = np.inf                                  # chain 2: NaN reductions, best_row 0
    X = nd_double(mex, np.transpose(chain, (2, 1, 0)))         # P x n x rows
    args = (cid.astype(np.float64) + 1.0, X, s2.T.copy())
    try:
        with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
            got = mex.call("chainlp", gw, *args, mu.T.copy(), sig.T.copy())[0]
            want = lk.chainlp(chain, s2, cid, mu, sig)
            same_struct(got, want, n, P, rows)
            assert got["best_row"][0].tolist()[1] == 0.0 and np.isnan(got["dic"][0, 1]) and np.all(got["best_row"][0, [0, 2]] >= 1)
            # the library's messages name the chain and the index
            bad = sig.copy()
            bad[2, 8] = 0.0
            e = expect("tci:call", mex.call, "chainlp", gw, *args, mu.T.copy(), bad.T.copy())
            assert "prior_sig of chain 2, index 8" in e.msg and str(_lib.TCI_EINVAL) in e.msg
            bad = mu.copy()
            bad[0, 3] = np.nan
            e = expect("tci:call", mex.call, "chainlp", gw, *args, bad.T.copy(), sig.T.copy())
            assert "prior_mu of chain 0, index 3" in e.msg
            e = expect("tci:call", mex.call, "chainlp", gw, np.array([1.0, 300.0, 2.0]), X, s2.T.copy(), mu.T.copy(), sig.T.copy())
            assert "cell id 299" in e.msg                       # cell 300 of 299
    finally:
        X.free()
        mex.call("destroy", gw, nlhs=0)
        gw.free()


@pytest.mark.gpu
def test_dram_logpost_equals_the_binding_bitwise(mex, cells):
    from transcriptioncycleinference_amd import Likelihood
    from transcriptioncycleinference_amd.mcmc import DramOptions, dram_run

    d = data_struct(mex, cells, range(cells.n_cells))
    h = mex.call("create", d, "P2P-MS2v5-LacZ-PP7v4", 0.0)[0]
    d.free()
    gw = MxPtr(mex, mex.handle(int(h[0, 0])))
    ids = [0, 17, 150]
    plan, a = _dram_args(mex, cells, ids)
    kv = dict(nsimu=300.0, burnintime=100.0, adaptint=50.0, thin=2.0, seed=13.0, logpost=True)
    try:
        with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
            do = DramOptions(n_steps=300, burnintime=100, adaptint=50, stats_from=100, thin=2, seed=13)
            want = dram_run(lk, np.asarray(plan.cells, np.int32), plan.x0, plan.lower, plan.upper, plan.prior_mu,
                            plan.prior_sig, plan.qcov_diag, 1.0, do, logpost=True, stats=True)
            n, P = plan.x0.shape
            for nlhs in (1, 3, 5):       # no chain output, the chain, the chain and the statistics
                o = _opts(mex, **kv)
                out = mex.call("dram", gw, *a, o, nlhs=nlhs)
                o.free()
                same_struct(out[0]["logpost"], want.lp, n, P, 100)
                np.testing.assert_array_equal(out[0]["mean"], want.mean.T)
                if nlhs >= 3:
                    np.testing.assert_array_equal(np.transpose(out[1], (2, 1, 0)), want.chain)
                if nlhs >= 5:
                    np.testing.assert_array_equal(out[4]["tau"], want.stats.tau.T)
            o = _opts(mex, **{**kv, "logpost": False})
            assert "logpost" not in mex.call("dram", gw, *a, o, nlhs=1)[0]
            o.free()
    finally:
        mex.call("destroy", gw, nlhs=0)
        gw.free()
