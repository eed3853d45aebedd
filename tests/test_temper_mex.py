"""The 'temper' and 'swap_every' options of tci_mex('dram', ...) through the stand-in MATLAB API: the checks that come
before the handle is touched (CPU) and, on the GPU, bitwise equality with the Python binding, in MATLAB's conventions:
options.temper is 2 x n [beta; ladder] with 1-based ladder numbers (0 = in no ladder), res.temper holds the per-chain
vectors 1 x n, the per-event logs n x n_events and event_rows 1 x n_events."""
import numpy as np
import pytest

from mexharness import MxPtr
from test_mex_gateway import _dram_args, _opts, data_struct, expect, mex  # noqa: F401  (mex: the gateway fixture)

IDS = [0, 0, 17, 17, 17, 150]
LADDER = np.array([1.0, 1.0, 2.0, 2.0, 2.0, 0.0])          # 1-based, 0 = none
BETA = np.array([1.0, 0.8, 1.0, 0.85, 0.7, 1.0])


def test_dram_temper_options_are_checked(mex, cells):
    fake = MxPtr(mex, mex.handle(12345))
    _, a = _dram_args(mex, cells, IDS)
    T = np.stack([BETA, LADDER])
    bad_ladder = T.copy()
    bad_ladder[1, 2] = 1.5
    neg_ladder = T.copy()
    neg_ladder[1, 0] = -1.0
    for kv, word in (({"temper": T[:, :5]}, "temper"), ({"temper": np.ones((3, 6))}, "temper"), ({"temper": "hot"}, "temper"),
                     ({"temper": bad_ladder}, "temper(2, 3)"), ({"temper": neg_ladder}, "temper(2, 1)"),
                     ({"temper": T, "swap_every": -1.0}, "swap_every"), ({"temper": T, "swap_every": 0.5}, "swap_every"),
                     ({"temper": T, "logpost": True}, "logpost")):
        o = _opts(mex, **kv)
        e = expect("tci:opts", mex.call, "dram", fake, *a, o)
        assert word in e.msg, (kv, e.msg)
        o.free()
    for kv in ({"temper": T}, {"temper": BETA}, {"temper": T, "swap_every": 0.0}, {"swap_every": 3.0}):
        o = _opts(mex, **kv)
        expect("tci:handle", mex.call, "dram", fake, *a, o)      # well-formed: only the handle is bad
        o.free()
    fake.free()


@pytest.mark.gpu
def test_dram_temper_equals_the_binding_bitwise(mex, cells):
    from transcriptioncycleinference_amd import Likelihood, _lib
    from transcriptioncycleinference_amd.mcmc import DramOptions, dram_run

    d = data_struct(mex, cells, range(cells.n_cells))
    h = mex.call("create", d, "P2P-MS2v5-LacZ-PP7v4", 0.0)[0]
    d.free()
    gw = MxPtr(mex, mex.handle(int(h[0, 0])))
    plan, a = _dram_args(mex, cells, IDS)
    kv = dict(nsimu=161.0, burnintime=40.0, adaptint=20.0, thin=2.0, seed=13.0, swap_every=2.0)
    T = np.stack([BETA, LADDER])
    try:
        with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
            do = DramOptions(n_steps=161, burnintime=40, adaptint=20, stats_from=40, thin=2, seed=13)
            run = lambda **k: dram_run(lk, np.asarray(plan.cells, np.int32), plan.x0, plan.lower, plan.upper,  # noqa: E731
                                       plan.prior_mu, plan.prior_sig, plan.qcov_diag, 1.0, do, **k)
            want = run(beta=BETA, ladder=LADDER.astype(np.int32) - 1, swap_every=2, stats=True)
            tr = want.temper
            assert tr.n_events == 4 and tr.swap_tried.sum() > 0
            n = len(IDS)
            for nlhs in (1, 3, 5):       # no chain output, the chain, the chain and the statistics
                o = _opts(mex, temper=T, **kv)
                out = mex.call("dram", gw, *a, o, nlhs=nlhs)
                o.free()
                got = out[0]["temper"]
                np.testing.assert_array_equal(got["beta"][0], BETA)
                np.testing.assert_array_equal(got["ladder"][0], LADDER)
                np.testing.assert_array_equal(got["swap_tried"][0], tr.swap_tried)
                np.testing.assert_array_equal(got["swap_accepted"][0], tr.swap_accepted)
                assert got["swap_logr"].shape == (n, 4) and got["swap_acc"].shape == (n, 4)
                assert np.ascontiguousarray(got["swap_logr"].T).tobytes() == tr.swap_logr.tobytes()
                np.testing.assert_array_equal(got["swap_acc"].T, tr.swap_acc)
                np.testing.assert_array_equal(got["event_rows"][0], tr.event_rows)
                assert got["n_events"][0, 0] == 4 and got["swap_every"][0, 0] == 2
                np.testing.assert_array_equal(out[0]["mean"], want.mean.T)
                np.testing.assert_array_equal(out[0]["sigma_mean"][0], want.sigma_mean)
                np.testing.assert_array_equal(out[0]["accept_rate"][0], want.accept_rate)
                np.testing.assert_array_equal(out[0]["final_theta"], want.final_theta.T)
                if nlhs >= 3:
                    np.testing.assert_array_equal(np.transpose(out[1], (2, 1, 0)), want.chain)
                    np.testing.assert_array_equal(out[2].T, want.s2chain)
                if nlhs >= 5:
                    np.testing.assert_array_equal(out[4]["tau"], want.stats.tau.T)
            # beta alone (1 x n): rungs without ladders, no swap is tried
            o = _opts(mex, temper=BETA, **kv)
            got = mex.call("dram", gw, *a, o, nlhs=1)[0]
            o.free()
            alone = run(beta=BETA, swap_every=2)
            np.testing.assert_array_equal(got["mean"], alone.mean.T)
            assert not got["temper"]["swap_tried"].any() and np.all(got["temper"]["ladder"] == 0)
            # without the option: no res.temper, the plain run
            o = _opts(mex, **kv)
            got = mex.call("dram", gw, *a, o, nlhs=1)[0]
            o.free()
            assert "temper" not in got
            np.testing.assert_array_equal(got["mean"], run().mean.T)
            # the library's refusals come through with its message
            bad = T.copy()
            bad[0, 1] = 1.0                                     # not decreasing along ladder 1 (0-based: ladder 0)
            o = _opts(mex, temper=bad, **kv)
            e = expect("tci:call", mex.call, "dram", gw, *a, o)
            o.free()
            assert "(ladder 0, chains 0 and 1)" in e.msg and str(_lib.TCI_EINVAL) in e.msg
    finally:
        mex.call("destroy", gw, nlhs=0)
        gw.free()
