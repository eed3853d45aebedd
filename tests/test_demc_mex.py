"""tci_mex('demc', ...) through the stand-in MATLAB API: the checks that come before the handle is touched (CPU) and, on
the GPU, bitwise equality with the Python binding, in MATLAB's conventions: a population is P x (n_pop * n), column
(k - 1) * n_pop + i member i of cells(k); chain comes back P x n_chains x n_keep, the kept vectors and the logs
n_chains x rows, pop P x n_pop x n, the per-member vectors n_pop x n."""
import numpy as np
import pytest

from mexharness import MxPtr
from test_mex_gateway import _opts, data_struct, expect, mex  # noqa: F401  (mex: the gateway fixture)
from test_modesearch_mex import search_args

IDS = [0, 17, 150]
N_POP, N_GEN, SEED = 6, 5, 13


def demc_args(cells):
    """(SearchPlan, jitter [K, P], [cells, POP0, LB, UB, MU, SIG, JIT]) as MATLAB holds them."""
    from transcriptioncycleinference_amd.mcmc import demc_jitter

    sp, a = search_args(cells, IDS, N_POP)
    jit = 20.0 * demc_jitter(cells, sp.cells)
    return sp, jit, a + [jit.T.copy()]


def test_demc_arguments_and_options_are_checked(mex, cells):
    fake = MxPtr(mex, mex.handle(12345))
    _, _, a = demc_args(cells)
    P = a[1].shape[0]
    expect("tci:handle", mex.call, "demc", fake, *a)                        # well-formed: only the handle is bad
    expect("tci:handle", mex.call, "demc", fake, *a, 2.0)
    expect("tci:handle", mex.call, "demc", fake, *a, np.ones(3), np.zeros((0, 0)))
    expect("tci:arg", mex.call, "demc", fake, *a[:6])                       # too few arguments: no JIT
    expect("tci:arg", mex.call, "demc", fake, a[0] - a[0], *a[1:])          # cells are 1-based
    expect("tci:arg", mex.call, "demc", fake, a[0], a[1][:, :-1], *a[2:])   # not n_pop columns per cell
    expect("tci:arg", mex.call, "demc", fake, *a, np.ones(2))               # sigma2: scalar or one per cell
    for k in range(3, 7):
        bad = list(a)
        bad[k] = a[k][:P - 1]
        e = expect("tci:arg", mex.call, "demc", fake, *bad)
        assert ("UB", "MU", "SIG", "JIT")[k - 3] in e.msg
    for ident, kv, word in (("tci:opts", {"n_gen": -1.0}, "n_gen"), ("tci:opts", {"thin": 2.5}, "thin"),
                            ("tci:opts", {"jump_every": -1.0}, "jump_every"), ("tci:opts", {"log_rows": -1.0}, "log_rows"),
                            ("tci:opts", {"seed": -1.0}, "seed"), ("tci:arg", {"keys": np.ones(2)}, "keys"),
                            ("tci:opts", {"keys": np.array([0.0, 1.5, 2.0])}, "keys(2)"),
                            ("tci:opts", {"F": 0.5}, "F")):
        o = _opts(mex, **kv)
        e = expect(ident, mex.call, "demc", fake, *a, 1.0, o)
        assert word in e.msg, (kv, e.msg)
        o.free()
    fake.free()


@pytest.mark.gpu
def test_demc_equals_the_binding_bitwise(mex, cells):
    from transcriptioncycleinference_amd import Likelihood, _lib

    ds = data_struct(mex, cells, range(cells.n_cells))
    h = mex.call("create", ds, "P2P-MS2v5-LacZ-PP7v4", 0.0)[0]
    ds.free()
    gw = MxPtr(mex, mex.handle(int(h[0, 0])))
    sp, jit, a = demc_args(cells)
    K = len(IDS)
    B = K * N_POP
    keys = np.array([7.0, 3.0, 40.0])
    try:
        with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
            cid = np.asarray(sp.cells, np.int32)
            run = lambda **k: lk.demc(sp.pop0, cid, sp.lower, sp.upper, sp.prior_mu, sp.prior_sig, jit,  # noqa: E731
                                      n_gen=N_GEN, seed=SEED, **k)

            def same(got, want, rows, logs):
                assert got["chain"].shape == (sp.pop0.shape[2], B, rows) and got["n_keep"][0, 0] == rows
                np.testing.assert_array_equal(np.transpose(got["chain"], (2, 1, 0)), want.chain)
                for f in ("s2chain", "sschain", "prichain"):
                    np.testing.assert_array_equal(got[f].T, getattr(want, f), err_msg=f)
                np.testing.assert_array_equal(np.transpose(got["pop"], (2, 1, 0)), want.pop)
                for f in ("s2", "ss", "accept_rate", "n_oob", "n_evals"):
                    np.testing.assert_array_equal(got[f].T, getattr(want, f), err_msg=f)
                assert got["logr"].shape == (B, logs)
                for f in ("logr", "accepted", "trial_oob"):
                    np.testing.assert_array_equal(got[f].T, getattr(want, f), err_msg=f)

            o = _opts(mex, n_gen=float(N_GEN), seed=float(SEED))
            got = mex.call("demc", gw, *a, 1.0, o)[0]
            o.free()
            same(got, run(), N_GEN + 1, 0)
            assert "rhat" not in got and "ess" not in got
            s2 = np.array([1.0, 2.0, 0.5])
            kw = dict(thin=2, jump_every=2, stats_from=2, CR=0.4, gamma0=1.5, log_rows=4, max_lag=2)
            o = _opts(mex, n_gen=float(N_GEN), seed=float(SEED), keys=keys, rhat=1.0, ess=1.0, updatesigma=0.0,
                      **{k: float(v) for k, v in kw.items()})
            want = run(sigma2_0=s2, keys=keys.astype(np.int64), rhat=True, ess=True, updatesigma=False, **kw)
            got = mex.call("demc", gw, *a, s2, o)[0]
            o.free()
            same(got, want, N_GEN // 2 + 1, 4)
            assert want.accepted.sum() > 0 and want.trial_oob.sum() > 0 and np.all(got["s2chain"].T == s2.repeat(N_POP))
            np.testing.assert_array_equal(got["rhat"].T, want.rhat.rhat)
            np.testing.assert_array_equal(got["s2_rhat"][0], want.rhat.s2_rhat)
            np.testing.assert_array_equal(got["ess"].T, want.ess.ess)
            np.testing.assert_array_equal(got["s2_ess"][0], want.ess.s2_ess)
            for k, c in enumerate(sp.cells):
                n = 7 + int(cells.lengths[c])
                assert got["rhat_max"][0, k] == np.nanmax(np.append(want.rhat.rhat[k, :n], want.rhat.s2_rhat[k]))
                assert got["ess_min"][0, k] == np.nanmin(np.append(want.ess.ess[k, :n], want.ess.s2_ess[k]))
            # the library's refusals come through with its message
            bad = a[1].copy()
            bad[5, N_POP + 2] = 1.5                                     # A of cell 2's member 3 above its bound
            e = expect("tci:call", mex.call, "demc", gw, a[0], bad, *a[2:])
            assert "cell 1, member 2, index 5" in e.msg and str(_lib.TCI_EINVAL) in e.msg
    finally:
        mex.call("destroy", gw, nlhs=0)
        gw.free()
