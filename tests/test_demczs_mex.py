"""tci_mex('demczs', ...) through the stand-in MATLAB API: the checks that come before the handle is touched (CPU) and,
on the GPU, bitwise equality with the Python binding, in MATLAB's conventions: POP0 is P x (n_pop * n) and Z0
P x (m0 * n), column (k - 1) * rows + i row i of cells(k); chain comes back P x n_chains x n_keep, the kept vectors and
the logs n_chains x rows, pop P x n_pop x n, archive P x n_archive x n, the per-chain vectors n_pop x n."""
import numpy as np
import pytest

from mexharness import MxPtr
from test_mex_gateway import _opts, data_struct, expect, mex  # noqa: F401  (mex: the gateway fixture)
from test_modesearch_mex import search_args

IDS = [0, 17, 150]
N_POP, M0, N_GEN, SEED = 3, 12, 6, 13


def zs_args(cells):
    """(SearchPlan of M0 members, jitter [K, P], [cells, POP0, Z0, LB, UB, MU, SIG, JIT]) as MATLAB holds them: the
    chains start at the archive's first N_POP rows."""
    from transcriptioncycleinference_amd.mcmc import demc_jitter

    sp, a = search_args(cells, IDS, M0)
    K, _, P = sp.pop0.shape
    jit = 20.0 * demc_jitter(cells, sp.cells)
    pop = sp.pop0[:, :N_POP].reshape(K * N_POP, P).T.copy()
    return sp, jit, [a[0], pop] + a[1:] + [jit.T.copy()]


def test_demczs_arguments_and_options_are_checked(mex, cells):
    fake = MxPtr(mex, mex.handle(12345))
    _, _, a = zs_args(cells)
    P = a[1].shape[0]
    expect("tci:handle", mex.call, "demczs", fake, *a)                        # well-formed: only the handle is bad
    expect("tci:handle", mex.call, "demczs", fake, *a, 2.0)
    expect("tci:handle", mex.call, "demczs", fake, *a, np.ones(3), np.zeros((0, 0)))
    expect("tci:arg", mex.call, "demczs", fake, *a[:7])                       # too few arguments: no JIT
    expect("tci:arg", mex.call, "demczs", fake, a[0] - a[0], *a[1:])          # cells are 1-based
    expect("tci:arg", mex.call, "demczs", fake, a[0], a[1][:, :-1], *a[2:])   # POP0: not n_pop columns per cell
    e = expect("tci:arg", mex.call, "demczs", fake, *a[:2], a[2][:, :-1], *a[3:])   # Z0: not m0 columns per cell
    assert "Z0" in e.msg
    expect("tci:arg", mex.call, "demczs", fake, *a, np.ones(2))               # sigma2: scalar or one per cell
    for k in range(4, 8):
        bad = list(a)
        bad[k] = a[k][:P - 1]
        e = expect("tci:arg", mex.call, "demczs", fake, *bad)
        assert ("UB", "MU", "SIG", "JIT")[k - 4] in e.msg
    for ident, kv, word in (("tci:opts", {"n_gen": -1.0}, "n_gen"), ("tci:opts", {"append_every": 0.0}, "append_every"),
                            ("tci:opts", {"append_every": 2.5}, "append_every"), ("tci:opts", {"log_rows": -1.0}, "log_rows"),
                            ("tci:arg", {"keys": np.ones(2)}, "keys"), ("tci:opts", {"F": 0.5}, "F"),
                            ("tci:arg", {"n_gen": float(2 ** 23), "append_every": 1.0}, "2^24")):
        o = _opts(mex, **kv)
        e = expect(ident, mex.call, "demczs", fake, *a, 1.0, o)
        assert word in e.msg, (kv, e.msg)
        o.free()
    o = _opts(mex, p_snooker=0.5)                                             # an option of 'demczs' alone
    e = expect("tci:opts", mex.call, "demc", fake, *a[:2], *a[3:], 1.0, o)
    assert "p_snooker" in e.msg
    o.free()
    fake.free()


@pytest.mark.gpu
def test_demczs_equals_the_binding_bitwise(mex, cells):
    from transcriptioncycleinference_amd import Likelihood, _lib

    ds = data_struct(mex, cells, range(cells.n_cells))
    h = mex.call("create", ds, "P2P-MS2v5-LacZ-PP7v4", 0.0)[0]
    ds.free()
    gw = MxPtr(mex, mex.handle(int(h[0, 0])))
    sp, jit, a = zs_args(cells)
    K = len(IDS)
    B = K * N_POP
    keys = np.array([7.0, 3.0, 40.0])
    try:
        with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
            cid = np.asarray(sp.cells, np.int32)
            run = lambda **k: lk.demczs(sp.pop0[:, :N_POP], sp.pop0, cid, sp.lower, sp.upper, sp.prior_mu,  # noqa: E731
                                        sp.prior_sig, jit, n_gen=N_GEN, seed=SEED, **k)

            def same(got, want, rows, logs):
                assert got["chain"].shape == (sp.pop0.shape[2], B, rows) and got["n_keep"][0, 0] == rows
                np.testing.assert_array_equal(np.transpose(got["chain"], (2, 1, 0)), want.chain)
                for f in ("s2chain", "sschain", "prichain"):
                    np.testing.assert_array_equal(got[f].T, getattr(want, f), err_msg=f)
                np.testing.assert_array_equal(np.transpose(got["pop"], (2, 1, 0)), want.pop)
                for f in ("s2", "ss", "accept_rate", "n_oob", "n_evals", "n_null"):
                    np.testing.assert_array_equal(got[f].T, getattr(want, f), err_msg=f)
                assert got["logr"].shape == (B, logs) and got["n_archive"][0, 0] == want.n_archive
                for f in ("logr", "accepted", "trial_oob", "ljac", "snooker"):
                    np.testing.assert_array_equal(got[f].T, getattr(want, f), err_msg=f)

            o = _opts(mex, n_gen=float(N_GEN), seed=float(SEED))
            got = mex.call("demczs", gw, *a, 1.0, o)[0]
            o.free()
            same(got, run(), N_GEN + 1, 0)
            assert "rhat" not in got and "ess" not in got and "archive" not in got
            s2 = np.array([1.0, 2.0, 0.5])
            kw = dict(thin=2, jump_every=2, stats_from=2, CR=0.4, gamma0=1.5, log_rows=5, max_lag=2, append_every=2,
                      p_snooker=0.5)
            o = _opts(mex, n_gen=float(N_GEN), seed=float(SEED), keys=keys, rhat=1.0, ess=1.0, updatesigma=0.0, archive=1.0,
                      **{k: float(v) for k, v in kw.items()})
            want = run(sigma2_0=s2, keys=keys.astype(np.int64), rhat=True, ess=True, updatesigma=False, archive=True, **kw)
            got = mex.call("demczs", gw, *a, s2, o)[0]
            o.free()
            same(got, want, N_GEN // 2 + 1, 5)
            assert want.accepted.sum() > 0 and 0 < want.snooker.sum() < want.snooker.size
            assert got["archive"].shape == (sp.pop0.shape[2], M0 + N_POP * 3, K)
            np.testing.assert_array_equal(np.transpose(got["archive"], (2, 1, 0)), want.archive)
            np.testing.assert_array_equal(got["rhat"].T, want.rhat.rhat)
            np.testing.assert_array_equal(got["s2_rhat"][0], want.rhat.s2_rhat)
            np.testing.assert_array_equal(got["ess"].T, want.ess.ess)
            np.testing.assert_array_equal(got["s2_ess"][0], want.ess.s2_ess)
            for k, c in enumerate(sp.cells):
                n = 7 + int(cells.lengths[c])
                assert got["rhat_max"][0, k] == np.nanmax(np.append(want.rhat.rhat[k, :n], want.rhat.s2_rhat[k]))
                assert got["ess_min"][0, k] == np.nanmin(np.append(want.ess.ess[k, :n], want.ess.s2_ess[k]))
            # the library's refusals come through with its message
            bad = a[2].copy()
            bad[5, M0 + 2] = 1.5                                        # A of cell 2's archive row 3 above its bound
            e = expect("tci:call", mex.call, "demczs", gw, *a[:2], bad, *a[3:])
            assert "z0 of cell 1, row 2, index 5" in e.msg and str(_lib.TCI_EINVAL) in e.msg
    finally:
        mex.call("destroy", gw, nlhs=0)
        gw.free()
