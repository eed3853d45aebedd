"""The DE-MC population sampler on the device (tci_demc_run / tci_demc.hip) against the numpy restatement
(tests/demc_oracle.py). The restatement takes Likelihood.ss_batch as its SS function, the same kernel and hence the same
bits, so every output is compared bit for bit; the one inexact step, u < exp(logr), must be decidable for every decision
of a replayed run (demc_oracle.EXP_MARGIN)."""
import numpy as np
import pytest

import chainlp_oracle as LPO
import demc_oracle as O

pytestmark = pytest.mark.gpu

CELLS = (290, 0, 219)        # TestData cells of 113, 120 and 129 points: P = 120, 127 and 136
SEED = 11
KEPT = ("chain", "s2chain", "sschain", "prichain")
MEMBER = ("pop", "s2", "ss", "accept_rate", "n_oob", "n_evals")
LOGS = ("logr", "accepted", "trial_oob")
S2_RTOL = 1e-9               # what tests/test_dram_gpu.py:709 holds the sampler's s2chain to against its restatement


@pytest.fixture(scope="module")
def lk(cells):
    from transcriptioncycleinference_amd import Likelihood

    assert tuple(int(cells.lengths[c]) for c in CELLS) == (113, 120, 129)
    with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as L:
        yield L


def population(cl, ids, n_pop, v0=None):
    from transcriptioncycleinference_amd import mcmc

    return mcmc.search_population(cl, ids, SEED, n_pop, v0=v0)


def jitter_of(cl, sp, scale=1.0):
    from transcriptioncycleinference_amd import mcmc

    jit = mcmc.demc_jitter(cl, sp.cells)
    out = np.zeros_like(sp.lower)
    out[:, :jit.shape[1]] = scale * jit
    return out


def device(lk, sp, jit, **kw):
    kw.setdefault("updatesigma", False)
    return lk.demc(sp.pop0, np.array(sp.cells, np.int32), sp.lower, sp.upper, sp.prior_mu, sp.prior_sig, jit, seed=SEED,
                   **kw)


def oracle_cell(lk, sp, jit, k, key, **kw):
    c = sp.cells[k]
    P = 7 + int(lk.cells.lengths[c])
    return O.run(lambda rows: lk.ss_batch(rows, np.full(len(rows), c, np.int32)), sp.pop0[k], P, sp.lower[k], sp.upper[k],
                 sp.prior_mu[k], sp.prior_sig[k], jit[k], key=key, seed=SEED, **kw)


def cell_view(got, f, k, n_pop):
    a = getattr(got, f)
    return a[:, k * n_pop:(k + 1) * n_pop] if f in KEPT + LOGS else a[k]


def assert_cell(got, k, want, n_pop, fields=KEPT + MEMBER + LOGS):
    for f in fields:
        g = cell_view(got, f, k, n_pop)
        np.testing.assert_array_equal(np.asarray(g), np.asarray(want[f]).reshape(np.shape(g)), err_msg=f"{f} of cell {k}")


@pytest.fixture(scope="module")
def replays(lk):
    """Every forced replay once: (n_pop, CR) -> (device run, the three cells' restatements). The jitter is 40 times the
    default, wide enough for proposals to leave the box."""
    out = {}
    for n_pop in (4, 5, 70):
        sp = population(lk.cells, CELLS, n_pop)
        jit = jitter_of(lk.cells, sp, 40.0)
        for CR in (0.0, 0.3, 1.0):
            kw = dict(n_gen=6, jump_every=3, thin=2, CR=CR)
            got = device(lk, sp, jit, log_rows=6, **kw)
            out[n_pop, CR] = got, [oracle_cell(lk, sp, jit, k, key=k, **kw) for k in range(3)]
    return out


@pytest.mark.parametrize("n_pop", [4, 5, 70])
@pytest.mark.parametrize("CR", [0.0, 0.3, 1.0])
def test_replay_bit_for_bit(replays, n_pop, CR):
    got, want = replays[n_pop, CR]
    assert got.chain.shape[:2] == (4, 3 * n_pop) and got.logr.shape == (6, 3 * n_pop)
    for k in range(3):
        assert want[k]["undecided"] == [], f"cell {k}: pick another seed"
        assert_cell(got, k, want[k], n_pop)
    assert np.all(got.n_evals == 7 - got.n_oob)


def test_the_replayed_runs_move(replays):
    acc = sum(int(g.accepted.sum()) for g, _ in replays.values())
    rej = sum(int((1 - g.accepted).sum()) for g, _ in replays.values())
    oob = sum(int(g.trial_oob.sum()) for g, _ in replays.values())
    print(f"replays: {acc} accepts, {rej} rejects, {oob} out of bounds")
    assert acc > 0 and rej > 0 and oob > 0
    for g, _ in replays.values():
        assert np.all(np.isnan(g.logr) == (g.trial_oob == 1)) and not np.any(g.accepted & g.trial_oob)


def test_sigma2_update_follows_the_restated_gamma_variate(lk):
    """updatesigma = 1: the restatement's decisions are forced on the device's own s2chain, and each of its s2 draws,
    Philox and Marsaglia-Tsang restated in Python, is held to the device's within S2_RTOL."""
    n_pop = 8
    sp = population(lk.cells, CELLS, n_pop)
    jit = jitter_of(lk.cells, sp)
    kw = dict(n_gen=6, jump_every=3, thin=1, CR=0.3, updatesigma=True)
    got = device(lk, sp, jit, log_rows=6, **kw)
    for k in range(3):
        forced = cell_view(got, "s2chain", k, n_pop)
        want = oracle_cell(lk, sp, jit, k, key=k, forced_s2=forced, **kw)
        assert want["undecided"] == []
        np.testing.assert_array_equal(forced[0], np.ones(n_pop))
        np.testing.assert_allclose(forced[1:], want["s2_draw"], rtol=S2_RTOL, atol=0)
        assert_cell(got, k, want, n_pop, fields=("chain", "sschain", "prichain", "pop", "ss", "accept_rate", "n_oob") + LOGS)
        assert len(np.unique(forced[1:])) == 6 * n_pop       # no two members share a Gamma stream
    fixed = device(lk, sp, jit, n_gen=6, thin=1, sigma2_0=[1.0, 2.5, 0.125])
    for k, s in enumerate((1.0, 2.5, 0.125)):
        assert np.all(cell_view(fixed, "s2chain", k, n_pop) == s) and np.all(fixed.s2[k] == s)


def test_a_cell_does_not_depend_on_its_neighbours_position_or_ld(lk):
    from transcriptioncycleinference_amd import mcmc

    n_pop = 8
    sp = population(lk.cells, CELLS, n_pop)
    jit = jitter_of(lk.cells, sp)
    kw = dict(n_gen=4, jump_every=3, thin=1, updatesigma=True, log_rows=4)
    together = device(lk, sp, jit, **kw)
    c, k = CELLS[0], 0
    P = 7 + int(lk.cells.lengths[c])
    two = population(lk.cells, (CELLS[2], c), n_pop)
    ld0 = two.pop0.shape[2]
    ld = ld0 + 5
    wide = lambda a, fill: np.concatenate([a, np.full(a.shape[:-1] + (ld - a.shape[-1],), fill)], axis=-1)  # noqa: E731
    sp2 = mcmc.SearchPlan(two.cells, wide(two.pop0, 7.0), wide(two.lower, -np.inf), wide(two.upper, np.inf),
                          wide(two.prior_mu, 0.0), wide(two.prior_sig, np.inf))
    alone = device(lk, sp2, wide(jitter_of(lk.cells, two), 0.0), keys=[5, k], **kw)
    for f in KEPT + MEMBER + LOGS:
        a, b = cell_view(alone, f, 1, n_pop), cell_view(together, f, k, n_pop)
        if f in ("chain", "pop"):
            a, b = a[..., :P], b[..., :P]
        np.testing.assert_array_equal(a, b, err_msg=f)
    assert np.all(alone.pop[1, :, ld0:] == 7.0) and np.all(alone.chain[:, n_pop:, ld0:] == 7.0)   # padding: the parent's
    one = population(lk.cells, (c,), n_pop)
    other = device(lk, one, jitter_of(lk.cells, one), keys=[9], **kw)
    assert not np.array_equal(other.pop[0], together.pop[k, :, :P])
    again = device(lk, one, jitter_of(lk.cells, one), keys=[k], **kw)
    np.testing.assert_array_equal(again.pop[0], together.pop[k, :, :P])   # ld = P here, 136 there
    np.testing.assert_array_equal(again.s2chain, cell_view(together, "s2chain", k, n_pop))


def test_kept_rows_stay_in_bounds_and_carry_their_own_ss_prior_and_reductions(lk):
    n_pop = 8
    sp = population(lk.cells, CELLS, n_pop)
    hier = population(lk.cells, (CELLS[1],), n_pop, v0={CELLS[1] + 1: 4.2})   # a hierarchical cell: v within 1e-5
    assert hier.lower[0, 0] == 4.2 - 1e-5 and hier.upper[0, 0] == 4.2 + 1e-5
    for plan in (sp, hier):
        jit = jitter_of(lk.cells, plan, 20.0)
        if plan is hier:
            from transcriptioncycleinference_amd import mcmc
            jit = np.zeros_like(plan.lower)
            jit[:, :] = 20.0 * mcmc.demc_jitter(lk.cells, plan.cells, v0={CELLS[1] + 1: 4.2})
        got = device(lk, plan, jit, n_gen=12, thin=2, jump_every=4, updatesigma=True, stats_from=4, rhat=True, ess=True)
        K = len(plan.cells)
        cid = np.repeat(np.array(plan.cells, np.int32), n_pop)
        rows, B, ld = got.chain.shape
        assert rows == 7 and B == K * n_pop
        np.testing.assert_array_equal(got.sschain.reshape(-1), lk.ss_batch(got.chain.reshape(-1, ld), np.tile(cid, rows)))
        for k, c in enumerate(plan.cells):
            P = 7 + int(lk.cells.lengths[c])
            x = got.chain[:, k * n_pop:(k + 1) * n_pop, :P]
            assert np.all(x >= plan.lower[k, :P]) and np.all(x <= plan.upper[k, :P])
            np.testing.assert_array_equal(got.prichain[:, k * n_pop:(k + 1) * n_pop].reshape(-1),
                                          LPO.pri(x.reshape(-1, P), plan.prior_mu[k, :P], plan.prior_sig[k, :P]))
        assert got.accepted is not None and got.accept_rate.sum() > 0
        np.testing.assert_array_equal(got.pop.reshape(B, ld), got.chain[-1])
        # the reductions: the stand-alone entry points on the returned chain, group = cell
        npar = 7 + lk.cells.lengths[cid]
        group = np.repeat(np.arange(K, dtype=np.int32), n_pop)
        cr = lk.chainrhat(got.chain[2:], got.s2chain[2:], npar=npar, group=group)
        ce = lk.chainess(got.chain[2:], got.s2chain[2:], npar=npar, group=group)
        assert got.rhat.n_rows == 5 and got.ess.n_rows == 5
        for f in ("rhat", "rhat_split", "pooled_mean", "pooled_std", "s2_rhat", "s2_pooled_std"):
            np.testing.assert_array_equal(getattr(got.rhat, f), getattr(cr, f), err_msg=f)
        for f in ("ess", "ess_split", "tau", "mcse", "window", "s2_ess"):
            np.testing.assert_array_equal(getattr(got.ess, f), getattr(ce, f), err_msg=f)


def test_the_sampler_targets_the_gaussian_it_is_given(lk):
    """demc_oracle.TARGET on the device: a likelihood flat to about 1e-8 in logr and a Gaussian prior on every
    coordinate; the pooled mean and std after burn-in within TARGET_Z Monte-Carlo standard errors of mu and sig."""
    c = CELLS[0]
    P = 7 + int(lk.cells.lengths[c])
    T = O.TARGET
    pop0, lo, up, mu, sig = O.gaussian_target(P, T["n_pop"], T["pop_seed"])
    got = lk.demc(pop0[None], [c], lo, up, mu, sig, T["jitter"] * sig, sigma2_0=T["sigma2_0"], n_gen=T["n_gen"], thin=1,
                  jump_every=0, CR=T["CR"], updatesigma=False, seed=T["seed"], keys=[c])
    z, ess = O.worst_z(got.chain[T["n_burn"]:], mu, sig)
    print(f"device: worst z {z:.3f}, least ESS {ess:.1f}, accept {got.accept_rate.mean():.3f}, {got.kernel_ms:.1f} ms")
    assert got.n_oob.sum() < 0.01 * got.n_evals.sum()
    assert z <= O.TARGET_Z


def test_refusals_name_the_offender_and_leave_the_context_usable(lk):
    from transcriptioncycleinference_amd import TciError, _lib, mcmc

    sp = population(lk.cells, CELLS, 4)
    jit = jitter_of(lk.cells, sp)

    def refused(code, *words, plan=sp, j=jit, **kw):
        with pytest.raises(TciError) as e:
            device(lk, plan, j, **{"n_gen": 1, **kw})
        assert e.value.code == code
        for w in words:
            assert w in str(e.value), str(e.value)
        device(lk, sp, jit, n_gen=1)   # a valid call on the same context succeeds

    cut = lambda p, **ch: mcmc.SearchPlan(**{**p.__dict__, **ch})  # noqa: E731
    refused(_lib.TCI_EINVAL, "n_pop", plan=cut(sp, pop0=sp.pop0[:, :3]))
    refused(_lib.TCI_EINVAL, "CR", CR=1.5)
    refused(_lib.TCI_EINVAL, "gamma0", gamma0=np.inf)
    refused(_lib.TCI_EINVAL, "jump_every", jump_every=-1)
    refused(_lib.TCI_EINVAL, "flags", flags=1)
    refused(_lib.TCI_EINVAL, "stats_from", stats_from=-1)
    bad = jit.copy()
    bad[1, 9] = -1.0
    refused(_lib.TCI_EINVAL, "jitter", "cell 1", "index 9", j=bad)
    refused(_lib.TCI_EINVAL, "sigma2_0", "cell 2", sigma2_0=[1.0, 1.0, 0.0])
    sg = sp.prior_sig.copy()
    sg[0, 3] = 0.0
    refused(_lib.TCI_EINVAL, "prior_sig", "cell 0", "index 3", plan=cut(sp, prior_sig=sg))
    out = sp.pop0.copy()
    out[1, 2, 5] = 1.5    # A above its upper bound 1
    refused(_lib.TCI_EINVAL, "cell 1", "member 2", "index 5", "outside", plan=cut(sp, pop0=out))
    nan = sp.pop0.copy()
    nan[2, 3, 40] = np.nan
    refused(_lib.TCI_EINVAL, "cell 2", "member 3", "index 40", "not finite", plan=cut(sp, pop0=nan))
    refused(_lib.TCI_EINVAL, "thin", thin=0, rhat=True)
    refused(_lib.TCI_EINVAL, "fewer than 2 kept rows", n_gen=4, thin=2, stats_from=4, rhat=True)
    refused(_lib.TCI_ERANGE, "cell 2", "136", plan=cut(sp, pop0=sp.pop0[:, :, :127], lower=sp.lower[:, :127],
                                                         upper=sp.upper[:, :127], prior_mu=sp.prior_mu[:, :127],
                                                         prior_sig=sp.prior_sig[:, :127]), j=jit[:, :127])


def test_refusals_the_binding_cannot_reach(lk):
    """The checks Python's own argument handling would intercept, or whose arrays it could not build, through the C entry
    point itself: sizes at or above 2^31, thin < 0, updatesigma outside {0, 1}, and TCI_ENOMEM with its byte count."""
    import ctypes as C

    from transcriptioncycleinference_amd import _lib

    sp = population(lk.cells, CELLS, 4)
    jit = jitter_of(lk.cells, sp)
    cid = np.array(sp.cells, np.int32)
    s20 = np.ones(3)
    P = lambda a: _lib.ptr(np.ascontiguousarray(a), _lib._dp)  # noqa: E731

    probe = np.empty(1)

    def call(n_sel=3, n_pop=4, kept=False, **o):
        opt = _lib.tci_demc_options()
        lk._lib.tci_demc_defaults(C.byref(opt))
        for k, v in o.items():
            setattr(opt, k, v)
        out = _lib.tci_demc_outputs()
        if kept:    # asks for the kept rows; only a run that cannot succeed may pass this one-element buffer
            out.sschain = _lib.ptr(probe, _lib._dp)
        rc = lk._lib.tci_demc_run(lk._h, C.byref(opt), P(sp.pop0), sp.pop0.shape[2], _lib.ptr(cid, _lib._i32p), n_sel, n_pop,
                                  P(sp.lower), P(sp.upper), P(sp.prior_mu), P(sp.prior_sig), P(jit), P(s20), C.byref(out),
                                  None, None, None, None)
        return rc, lk._lib.tci_last_error(lk._h).decode()

    assert call(n_gen=1)[0] == _lib.TCI_OK
    rc, msg = call(n_sel=2 ** 29, n_pop=4)
    assert rc == _lib.TCI_EINVAL and "n_sel * n_pop must stay below 2^31" in msg
    rc, msg = call(n_gen=2 ** 31 - 1)
    assert rc == _lib.TCI_EINVAL and "n_gen must stay below 2^31" in msg
    rc, msg = call(thin=-1)
    assert rc == _lib.TCI_EINVAL and "thin must be >= 0" in msg
    rc, msg = call(updatesigma=2)
    assert rc == _lib.TCI_EINVAL and "updatesigma must be 0 or 1" in msg
    # a device chain of 2^26 + 1 rows x 12 chains x (136 + 3) doubles: about 0.9 TB, more than the device has
    rc, msg = call(n_gen=2 ** 26, thin=1, kept=True)
    want = ((2 ** 26 + 1) * 12 * (136 + 3) + (12 + 6) * 136) * 8
    assert rc == _lib.TCI_ENOMEM and str(want) in msg and "do not fit the device" in msg, msg
    assert call(n_gen=1)[0] == _lib.TCI_OK     # the context is still usable


def test_fit_with_demc_pools_the_members_and_none_is_todays_fit(lk):
    from transcriptioncycleinference_amd import mcmc

    a, b = CELLS[0], CELLS[1]
    kw = dict(cells=[a, b], n_steps=300, n_burn=1, thin=1, seed=3)
    plain, none = mcmc.fit(lk, **kw), mcmc.fit(lk, demc=None, **kw)
    assert plain.MCMCdemc is None and none.MCMCdemc is None
    for x, y in zip(plain.MCMCchain, none.MCMCchain):
        for f in mcmc.CHAIN_FIELDS:
            np.testing.assert_array_equal(x[f], y[f])
    fr = mcmc.fit(lk, cells=[a, b], n_burn=4, thin=2, seed=3, demc=dict(n_pop=8, n_gen=12))
    res, sp = mcmc.demc(lk, n_pop=8, n_gen=12, thin=2, n_burn=4, seed=3, cells=[a, b])
    assert [set(e) for e in fr.MCMCdemc] == [set(mcmc.DEMC_FIELDS)] * 2
    for k, c in enumerate((a, b)):
        n = int(lk.cells.lengths[c])
        e = fr.MCMCdemc[k]
        assert e["cell_index"] == c + 1 and e["n_pop"] == 8 and e["n_gen"] == 12
        np.testing.assert_array_equal(e["accept_rate"], res.accept_rate[k])
        assert e["rhat_max"] == np.nanmax(np.append(res.rhat.rhat[k, :7 + n], res.rhat.s2_rhat[k]))
        assert e["ess_min"] == np.nanmin(np.append(res.ess.ess[k, :7 + n], res.ess.s2_ess[k]))
        pooled = res.chain[2:, k * 8:(k + 1) * 8, :7 + n].reshape(-1, 7 + n)
        np.testing.assert_array_equal(fr.MCMCchain[k]["v_chain"], pooled[:, 0])
        np.testing.assert_allclose([fr.MCMCresults[k]["mean_v"], fr.MCMCresults[k]["sigma_v"]],
                                   [pooled[:, 0].mean(), pooled[:, 0].std()], rtol=1e-12)
        np.testing.assert_array_equal(fr.final_theta[k], res.pop[k, 0])
        sq = res.s2chain[2:, k * 8:(k + 1) * 8].reshape(-1)        # sigma's summaries: the rows past burn-in too
        np.testing.assert_allclose([fr.MCMCresults[k]["mean_sigma"], fr.MCMCresults[k]["sigma_sigma"]],
                                   [np.sqrt(sq.mean()), np.sqrt(sq).std()], rtol=1e-12)
        np.testing.assert_array_equal(fr.MCMCchain[k]["s2chain"], res.s2chain[:, k * 8:(k + 1) * 8].reshape(-1))
    # from a mode search's final population, keyed by the dataset-wide cell index
    sr = mcmc.modesearch(lk, n_pop=8, n_gen=5, seed=3, cells=[a, b])
    pre, _ = mcmc.demc(lk, n_pop=8, n_gen=2, seed=3, cells=[a, b], presearch=dict(n_gen=5), rhat=False, ess=False)
    np.testing.assert_array_equal(pre.chain[0].reshape(2, 8, -1), sr[0].pop)
    shard, _ = mcmc.demc(lk, n_pop=8, n_gen=12, thin=2, n_burn=4, seed=3, cells=[b])
    np.testing.assert_array_equal(shard.pop[0, :, :7 + int(lk.cells.lengths[b])], res.pop[1, :, :7 + int(lk.cells.lengths[b])])
