"""tci_mex('chainrank', ...) through the stand-in MATLAB API: argument checks (CPU; they come before the handle is
touched) and, on the GPU, bitwise equality with the Python binding, in MATLAB's conventions: chain is P x n x rows,
the outputs are P x n_groups (q: P x nq x n_groups; the windows as doubles), group is 1-based (0 = in no group)."""
import numpy as np
import pytest

import chainess_oracle as E
from mexharness import MxPtr
from test_mex_gateway import data_struct, expect, mex  # noqa: F401  (mex: the gateway fixture)
from test_predict_mex import nd_double

DOUBLES = ("rhat_bulk", "rhat_folded", "rhat_rank", "ess_bulk", "tau_bulk", "ess_tail_lo", "ess_tail_hi", "ess_tail")
WINDOWS = ("window_bulk", "window_tail_lo", "window_tail_hi")


def test_chainrank_arguments_are_checked(mex):
    fake = MxPtr(mex, mex.handle(12345))
    X = nd_double(mex, np.zeros((9, 2, 30)))
    none = np.zeros((0, 0))
    try:
        expect("tci:handle", mex.call, "chainrank", fake, X, np.array([9.0, 9.0]), np.array([1.0, 1.0]))  # only the handle
        expect("tci:handle", mex.call, "chainrank", fake, X, none, none, 5.0, np.array([0.1, 0.9]), np.array([0.2, 0.8]))
        expect("tci:handle", mex.call, "chainrank", fake, X, none, none, none, none, none)     # [] = the defaults
        expect("tci:arg", mex.call, "chainrank", fake, X, none)                                # too few arguments
        expect("tci:arg", mex.call, "chainrank", fake, X, none, none, 0.0, none, none, 0.0)    # too many
        expect("tci:arg", mex.call, "chainrank", fake, X, none, none, -1.0)                    # max_lag >= 0
        expect("tci:arg", mex.call, "chainrank", fake, X, none, none, 1.5)
        expect("tci:arg", mex.call, "chainrank", fake, X, none, none, 0.0, np.array([0.5, 1.5]))   # a prob in [0, 1]
        expect("tci:arg", mex.call, "chainrank", fake, X, none, none, 0.0, np.full(17, 0.5))       # at most 16
        expect("tci:arg", mex.call, "chainrank", fake, X, none, none, 0.0, none, np.array([0.6, 0.5]))  # lo < hi
        expect("tci:arg", mex.call, "chainrank", fake, X, none, none, 0.0, none, np.array([0.0, 0.5]))  # 0 < lo
        expect("tci:arg", mex.call, "chainrank", fake, X, np.array([10.0, 1.0]), none)         # npar <= P
        expect("tci:arg", mex.call, "chainrank", fake, X, none, np.array([1.0, 3.0]))          # group <= n
        expect("tci:arg", mex.call, "chainrank", fake, X, none, np.array([0.0, 0.0]))          # no group at all
    finally:
        X.free()
        fake.free()


@pytest.mark.gpu
def test_chainrank_equals_the_binding_bitwise(mex, cells):
    from transcriptioncycleinference_amd import Likelihood

    d = data_struct(mex, cells, range(cells.n_cells))
    h = mex.call("create", d, "P2P-MS2v5-LacZ-PP7v4", 0.0)[0]
    d.free()
    gw = MxPtr(mex, mex.handle(int(h[0, 0])))
    rows, n, P = 257, 6, 37
    group = np.array([1, 0, 1, -1, 0, 1], np.int32)
    npar = np.array([16, 37, 16, 33, 37, 16], np.int32)
    chain, _ = E.ar1_chains(21, rows, n, P, npar)
    X = nd_double(mex, np.transpose(chain, (2, 1, 0)))       # P x n x rows
    try:
        with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
            for lag, probs, tail in ((None, None, None), (65.0, (0.1, 0.5), (0.2, 0.7))):
                extra = () if lag is None else (lag, np.array(probs), np.array(tail))
                got = mex.call("chainrank", gw, X, npar.astype(np.float64), (group + 1).astype(np.float64), *extra)[0]
                kw = {} if lag is None else dict(max_lag=int(lag), probs=probs, tail=tail)
                want = lk.chainrank(chain, None, npar, group, **kw)
                assert got["n_rows"][0, 0] == rows
                nq = want.q.shape[1]
                assert got["q"].shape == (P, nq, 2) and got["q_tail"].shape == (P, 2, 2)
                for k in ("q", "q_tail"):
                    assert np.ascontiguousarray(np.transpose(got[k], (2, 1, 0))).tobytes() == getattr(want, k).tobytes(), k
                for k in DOUBLES:
                    assert got[k].shape == (P, 2)
                    assert np.ascontiguousarray(got[k].T).tobytes() == getattr(want, k).tobytes(), k
                for k in WINDOWS:
                    assert np.array_equal(got[k].T, getattr(want, k).astype(np.float64)), k
            bare = mex.call("chainrank", gw, X, np.zeros((0, 0)), np.zeros((0, 0)))[0]
            assert bare["rhat_rank"].shape == (P, 1)
            assert np.ascontiguousarray(bare["rhat_rank"].T).tobytes() == lk.chainrank(chain).rhat_rank.tobytes()
    finally:
        X.free()
        mex.call("destroy", gw, nlhs=0)
        gw.free()


def same_rank_struct(got, want, P):
    """res.rank of a sampler command against a ChainRank: MATLAB's P x . x n_groups against [group][.][P]."""
    ng = want.q.shape[0]
    assert got["n_rows"][0, 0] == want.n_rows and got["q"].shape == (P, want.q.shape[1], ng)
    for k in ("q", "q_tail"):
        np.testing.assert_array_equal(np.transpose(got[k].reshape(P, -1, ng), (2, 1, 0)), getattr(want, k), err_msg=k)
        np.testing.assert_array_equal(got["s2_" + k].reshape(-1, ng).T, getattr(want, "s2_" + k), err_msg=k)
    for k in DOUBLES + WINDOWS:
        np.testing.assert_array_equal(got[k].reshape(P, ng).T, getattr(want, k).astype(np.float64), err_msg=k)
        np.testing.assert_array_equal(got["s2_" + k].reshape(ng), getattr(want, "s2_" + k).astype(np.float64), err_msg=k)


def test_options_rank_is_checked_before_the_handle(mex, cells):
    from test_demc_mex import demc_args
    from test_mex_gateway import _dram_args, _opts

    fake = MxPtr(mex, mex.handle(12345))
    _, a = _dram_args(mex, cells, [0, 1, 2])
    for kv, word in (({"rank": 1.0, "thin": 0.0}, "thin"), ({"rank": 1.0, "logpost": 1.0}, "logpost"),
                     ({"rank": 1.0, "temper": np.ones((1, 3))}, "temper"), ({"rank": [1.0, 0.0]}, "rank")):
        o = _opts(mex, **kv)
        e = expect("tci:opts" if word != "rank" else "tci:arg", mex.call, "dram", fake, *a, o)
        assert word in e.msg, (kv, e.msg)
        o.free()
    for kv in ({"rank": 1.0}, {"rank": 0.0}):
        o = _opts(mex, **kv)
        expect("tci:handle", mex.call, "dram", fake, *a, o)
        o.free()
    _, _, d = demc_args(cells)
    o = _opts(mex, rank=1.0, n_gen=4.0)
    expect("tci:handle", mex.call, "demc", fake, *d, 1.0, o)
    o.free()
    fake.free()


@pytest.mark.gpu
def test_options_rank_of_dram_and_demc_equal_the_binding_bitwise(mex, cells):
    from test_demc_mex import N_POP, demc_args
    from test_mex_gateway import _dram_args, _opts
    from transcriptioncycleinference_amd import Likelihood
    from transcriptioncycleinference_amd.mcmc import DramOptions, dram_run

    ds = data_struct(mex, cells, range(cells.n_cells))
    h = mex.call("create", ds, "P2P-MS2v5-LacZ-PP7v4", 0.0)[0]
    ds.free()
    gw = MxPtr(mex, mex.handle(int(h[0, 0])))
    try:
        with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
            # 'dram': cells 3, 41, 3, 41, 3: the chains of one cell form a group, numbered by first appearance
            ids = [3, 41, 3, 41, 3]
            plan, a = _dram_args(mex, cells, ids)
            keys = np.arange(5, dtype=np.int64) * 7 + 2
            o = _opts(mex, nsimu=400.0, burnintime=100.0, thin=1.0, seed=5.0, max_lag=30.0, rank=1.0,
                      chain_keys=keys.astype(np.float64))
            res = mex.call("dram", gw, *a, o, nlhs=1)[0]
            o.free()
            group = np.array([0, 1, 0, 1, 0], np.int32)
            want = dram_run(lk, np.asarray(plan.cells, np.int32), plan.x0, plan.lower, plan.upper, plan.prior_mu,
                            plan.prior_sig, plan.qcov_diag, 1.0,
                            DramOptions(n_steps=400, burnintime=100, stats_from=100, thin=1, seed=5), chain_keys=keys,
                            group=group, rank=True, max_lag=30)
            np.testing.assert_array_equal(res["mean"], want.mean.T)
            np.testing.assert_array_equal(res["rank"]["group"].reshape(-1), group + 1.0)
            same_rank_struct(res["rank"], want.rank, plan.x0.shape[1])
            # 'demc': a cell's members
            sp, jit, d = demc_args(cells)
            o = _opts(mex, n_gen=12.0, seed=13.0, stats_from=2.0, max_lag=4.0, rank=1.0)
            got = mex.call("demc", gw, *d, 1.0, o)[0]
            o.free()
            dm = lk.demc(sp.pop0, np.asarray(sp.cells, np.int32), sp.lower, sp.upper, sp.prior_mu, sp.prior_sig, jit,
                         n_gen=12, seed=13, stats_from=2, max_lag=4, rank=True)
            np.testing.assert_array_equal(np.transpose(got["chain"], (2, 1, 0)), dm.chain)
            assert "rhat" not in got and "ess" not in got
            np.testing.assert_array_equal(got["rank"]["group"].reshape(-1), np.repeat(np.arange(len(sp.cells)), N_POP) + 1.0)
            same_rank_struct(got["rank"], dm.rank, sp.pop0.shape[2])
    finally:
        mex.call("destroy", gw, nlhs=0)
        gw.free()
