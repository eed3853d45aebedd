"""The DE-MC(zs) sampler on the device (tci_demczs_run / tci_demczs.hip) against the numpy restatement
(tests/demczs_oracle.py). The restatement takes Likelihood.ss_batch as its SS function, the same kernel and hence the
same bits; its own ljac is held to the device's within the bound derived in the oracle's docstring and then replaced by
the device's bits, so every other output is compared bit for bit; the one inexact decision, u < exp(logr), must be
decidable for every decision of a replayed run (demc_oracle.EXP_MARGIN)."""
import dataclasses

import numpy as np
import pytest

import chainlp_oracle as LPO
import demc_oracle as D
import demczs_oracle as O

pytestmark = pytest.mark.gpu

CELLS = (290, 0, 219)        # TestData cells of 113, 120 and 129 points: P = 120, 127 and 136
SEED = 11
KEPT = ("chain", "s2chain", "sschain", "prichain")
MEMBER = ("pop", "s2", "ss", "accept_rate", "n_oob", "n_evals", "n_null")
LOGS = ("logr", "accepted", "trial_oob", "ljac", "snooker")
S2_RTOL = 1e-9               # what tests/test_dram_gpu.py holds the sampler's s2chain to against its restatement
SHAPES = [(1, 3), (3, 3), (5, 40), (70, 90)]
BIG = (1100, 1200)           # past the decision kernel's 1,024 threads


@pytest.fixture(scope="module")
def lk(cells):
    from transcriptioncycleinference_amd import Likelihood

    assert tuple(int(cells.lengths[c]) for c in CELLS) == (113, 120, 129)
    with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as L:
        yield L


@dataclasses.dataclass
class Plan:
    cells: tuple
    pop0: np.ndarray
    z0: np.ndarray
    lower: np.ndarray
    upper: np.ndarray
    prior_mu: np.ndarray
    prior_sig: np.ndarray
    jit: np.ndarray


_plans = {}


def plan(cl, ids, n_pop, m0, scale=1.0, v0=None):
    """The starts of n_pop chains and an archive of m0 rows per cell from search_population: the chains start at the
    archive's first rows, and with m0 < n_pop the archive holds the first chains' rows (m0 = 3: pop0's own rows)."""
    from transcriptioncycleinference_amd import mcmc

    key = (tuple(ids), n_pop, m0, scale, None if v0 is None else tuple(v0.items()))
    if key not in _plans:
        sp = mcmc.search_population(cl, ids, SEED, max(n_pop, m0), v0=v0)
        jit = np.zeros_like(sp.lower)
        base = mcmc.demc_jitter(cl, sp.cells, v0=v0)
        jit[:, :base.shape[1]] = scale * base
        _plans[key] = Plan(tuple(sp.cells), sp.pop0[:, :n_pop].copy(), sp.pop0[:, :m0].copy(), sp.lower, sp.upper,
                           sp.prior_mu, sp.prior_sig, jit)
    return _plans[key]


def device(lk, pl, **kw):
    kw.setdefault("updatesigma", False)
    kw.setdefault("seed", SEED)
    return lk.demczs(pl.pop0, pl.z0, np.array(pl.cells, np.int32), pl.lower, pl.upper, pl.prior_mu, pl.prior_sig, pl.jit,
                     **kw)


def oracle_cell(lk, pl, k, key, got=None, n_pop=None, **kw):
    c = pl.cells[k]
    P = 7 + int(lk.cells.lengths[c])
    if got is not None:
        kw["forced_ljac"] = cell_view(got, "ljac", k, n_pop)
    kw.pop("log_rows", None)
    kw.pop("archive", None)
    return O.run(lambda rows: lk.ss_batch(rows, np.full(len(rows), c, np.int32)), pl.pop0[k], pl.z0[k], P, pl.lower[k],
                 pl.upper[k], pl.prior_mu[k], pl.prior_sig[k], pl.jit[k], key=key, seed=SEED, **kw)


def cell_view(got, f, k, n_pop):
    a = getattr(got, f)
    return a[:, k * n_pop:(k + 1) * n_pop] if f in KEPT + LOGS else a[k]


def assert_cell(got, k, want, n_pop, fields=KEPT + MEMBER + LOGS + ("archive",)):
    for f in fields:
        g = cell_view(got, f, k, n_pop)
        np.testing.assert_array_equal(np.asarray(g), np.asarray(want[f]).reshape(np.shape(g)), err_msg=f"{f} of cell {k}")


def assert_ljac(got, k, want, n_pop):
    """The restatement's own ljac against the device's: within the derived bound where it is finite, the same value
    where it is not (-Inf for D' = 0); NaN, a move that was not an evaluated snooker move, is assert_cell's to compare."""
    dev, own, bnd = cell_view(got, "ljac", k, n_pop), want["ljac_own"], want["ljac_bound"]
    fin = np.isfinite(own)
    assert np.all(np.isfinite(dev[fin])) and np.all(bnd[fin] > 0)
    worst = np.max(np.abs(dev[fin] - own[fin]) / bnd[fin], initial=0.0)
    assert worst <= 1.0, f"cell {k}: ljac off by {worst:.2f} bounds"
    inf = np.isinf(own)
    np.testing.assert_array_equal(dev[inf], own[inf])
    return int(fin.sum())


_replays = {}


def replay(lk, n_pop, m0, p_snooker, append_every):
    """One forced replay, computed once: (device run, the three cells' restatements). The jitter is 40 times the
    default, wide enough for proposals to leave the box."""
    key = (n_pop, m0, p_snooker, append_every)
    if key not in _replays:
        pl = plan(lk.cells, CELLS, n_pop, m0, 40.0)
        kw = dict(n_gen=6, jump_every=3, thin=2, CR=0.3, p_snooker=p_snooker, append_every=append_every)
        got = device(lk, pl, log_rows=6, archive=True, **kw)
        _replays[key] = got, [oracle_cell(lk, pl, k, key=k, got=got, n_pop=n_pop, **kw) for k in range(3)]
    return _replays[key]


def check_replay(got, want, n_pop, m0, append_every):
    assert got.chain.shape[:2] == (4, 3 * n_pop) and got.logr.shape == (6, 3 * n_pop)
    assert got.n_archive == m0 + n_pop * (6 // append_every) == got.archive.shape[1]
    for k in range(3):
        assert want[k]["undecided"] == [], f"cell {k}: pick another seed"
        assert_ljac(got, k, want[k], n_pop)
        assert_cell(got, k, want[k], n_pop)
    assert np.all(got.n_evals == 7 - got.n_oob - got.n_null)


@pytest.mark.parametrize("append_every", [1, 2])
@pytest.mark.parametrize("p_snooker", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("n_pop,m0", SHAPES)
def test_replay_bit_for_bit(lk, n_pop, m0, p_snooker, append_every):
    got, want = replay(lk, n_pop, m0, p_snooker, append_every)
    check_replay(got, want, n_pop, m0, append_every)
    snk = got.snooker.mean()
    assert snk == p_snooker if p_snooker in (0.0, 1.0) else 0 < snk < 1


def test_replay_past_the_decision_kernels_threads(lk):
    got, want = replay(lk, *BIG, 0.5, 2)
    check_replay(got, want, *BIG, 2)
    assert 0.4 < got.snooker.mean() < 0.6


def test_the_replayed_runs_move(lk):
    runs = [replay(lk, n_pop, m0, p, ae)[0] for n_pop, m0 in SHAPES for p in (0.0, 0.5, 1.0) for ae in (1, 2)]
    runs.append(replay(lk, *BIG, 0.5, 2)[0])
    acc = sum(int(g.accepted.sum()) for g in runs)
    rej = sum(int((1 - g.accepted).sum()) for g in runs)
    oob = sum(int((g.trial_oob == 1).sum()) for g in runs)
    null = sum(int((g.trial_oob == 2).sum()) for g in runs)
    snk_acc = sum(int((g.accepted & g.snooker).sum()) for g in runs)
    print(f"replays: {acc} accepts ({snk_acc} of snooker moves), {rej} rejects, {oob} out of bounds, {null} null moves")
    assert acc > 0 and rej > 0 and oob > 0 and snk_acc > 0 and null > 0
    for g in runs:
        assert np.all(np.isnan(g.logr) == (g.trial_oob != 0)) and not np.any(g.accepted & (g.trial_oob != 0))
        assert np.all(g.snooker[g.trial_oob == 2] == 1) and np.all(g.ljac[g.snooker == 0] == 0)
        assert np.all(np.isnan(g.ljac) == ((g.snooker == 1) & (g.trial_oob != 0)))
        assert g.n_null.sum() >= (g.trial_oob == 2).sum() and np.all(g.n_oob.reshape(-1) == (g.trial_oob == 1).sum(axis=0))


def test_archive_is_z0_followed_by_the_chains_rows_at_the_append_generations(lk):
    n_pop, m0 = 5, 40
    pl = plan(lk.cells, CELLS, n_pop, m0)
    for ae in (1, 3):
        got = device(lk, pl, n_gen=7, thin=ae, append_every=ae, p_snooker=0.5, updatesigma=True, archive=True)
        q = 7 // ae
        assert got.archive.shape == (3, m0 + n_pop * q, pl.z0.shape[2]) and got.chain.shape[0] == q + 1
        for k in range(3):
            np.testing.assert_array_equal(got.archive[k, :m0], pl.z0[k])
            np.testing.assert_array_equal(got.archive[k, m0:].reshape(q, n_pop, -1),
                                          got.chain[1:, k * n_pop:(k + 1) * n_pop])
    assert device(lk, pl, n_gen=7, append_every=3).archive is None


def test_sigma2_update_follows_the_restated_gamma_variate(lk):
    """updatesigma = 1: the restatement's decisions are forced on the device's own s2chain, and each of its s2 draws,
    Philox and Marsaglia-Tsang restated in Python, is held to the device's within S2_RTOL."""
    n_pop, m0 = 4, 40
    pl = plan(lk.cells, CELLS, n_pop, m0)
    kw = dict(n_gen=6, jump_every=3, thin=1, CR=0.3, updatesigma=True, p_snooker=0.5, append_every=2)
    got = device(lk, pl, log_rows=6, archive=True, **kw)
    for k in range(3):
        forced = cell_view(got, "s2chain", k, n_pop)
        want = oracle_cell(lk, pl, k, key=k, got=got, n_pop=n_pop, forced_s2=forced, **kw)
        assert want["undecided"] == []
        np.testing.assert_array_equal(forced[0], np.ones(n_pop))
        np.testing.assert_allclose(forced[1:], want["s2_draw"], rtol=S2_RTOL, atol=0)
        assert_ljac(got, k, want, n_pop)
        assert_cell(got, k, want, n_pop, fields=("chain", "sschain", "prichain", "pop", "ss", "accept_rate", "n_oob",
                                                 "n_null", "archive") + LOGS)
        assert len(np.unique(forced[1:])) == 6 * n_pop       # no two chains share a Gamma stream
    fixed = device(lk, pl, n_gen=6, thin=1, sigma2_0=[1.0, 2.5, 0.125])
    for k, s in enumerate((1.0, 2.5, 0.125)):
        assert np.all(cell_view(fixed, "s2chain", k, n_pop) == s) and np.all(fixed.s2[k] == s)


def test_a_cell_does_not_depend_on_its_neighbours_position_ld_or_n_sel(lk):
    n_pop, m0 = 4, 30
    pl = plan(lk.cells, CELLS, n_pop, m0)
    kw = dict(n_gen=5, jump_every=3, thin=1, updatesigma=True, log_rows=5, p_snooker=0.5, append_every=2, archive=True)
    together = device(lk, pl, **kw)
    c, k = CELLS[0], 0
    P = 7 + int(lk.cells.lengths[c])
    two = plan(lk.cells, (CELLS[2], c), n_pop, m0)
    ld0 = two.pop0.shape[2]
    ld = ld0 + 5
    wide = lambda a, fill: np.concatenate([a, np.full(a.shape[:-1] + (ld - a.shape[-1],), fill)], axis=-1)  # noqa: E731
    pl2 = Plan(two.cells, wide(two.pop0, 7.0), wide(two.z0, 9.0), wide(two.lower, -np.inf), wide(two.upper, np.inf),
               wide(two.prior_mu, 0.0), wide(two.prior_sig, np.inf), wide(two.jit, 0.0))
    alone = device(lk, pl2, keys=[5, k], **kw)
    for f in KEPT + MEMBER + LOGS + ("archive",):
        a, b = cell_view(alone, f, 1, n_pop), cell_view(together, f, k, n_pop)
        if f in ("chain", "pop", "archive"):
            a, b = a[..., :P], b[..., :P]
        np.testing.assert_array_equal(a, b, err_msg=f)
    assert np.all(alone.pop[1, :, ld0:] == 7.0) and np.all(alone.chain[:, n_pop:, ld0:] == 7.0)   # padding: the parent's
    assert np.all(alone.archive[1, :m0, ld0:] == 9.0) and np.all(alone.archive[1, m0:, ld0:] == 7.0)
    one = plan(lk.cells, (c,), n_pop, m0)
    other = device(lk, one, keys=[9], **kw)
    assert not np.array_equal(other.pop[0], together.pop[k, :, :P])
    again = device(lk, one, keys=[k], **kw)
    np.testing.assert_array_equal(again.pop[0], together.pop[k, :, :P])   # ld = P and n_sel = 1 here, 136 and 3 there
    np.testing.assert_array_equal(again.s2chain, cell_view(together, "s2chain", k, n_pop))
    np.testing.assert_array_equal(again.ljac, cell_view(together, "ljac", k, n_pop))


def test_kept_rows_stay_in_bounds_and_carry_their_own_ss_prior_and_reductions(lk):
    n_pop, m0 = 4, 40
    v0 = {CELLS[1] + 1: 4.2}
    hier = plan(lk.cells, (CELLS[1],), n_pop, m0, 20.0, v0=v0)   # a hierarchical cell: v within 1e-5
    assert hier.lower[0, 0] == 4.2 - 1e-5 and hier.upper[0, 0] == 4.2 + 1e-5
    for pl in (plan(lk.cells, CELLS, n_pop, m0, 20.0), hier):
        got = device(lk, pl, n_gen=12, thin=2, jump_every=4, updatesigma=True, stats_from=4, rhat=True, ess=True, rank=True,
                     p_snooker=0.3, append_every=3)
        K = len(pl.cells)
        cid = np.repeat(np.array(pl.cells, np.int32), n_pop)
        rows, B, ld = got.chain.shape
        assert rows == 7 and B == K * n_pop
        np.testing.assert_array_equal(got.sschain.reshape(-1), lk.ss_batch(got.chain.reshape(-1, ld), np.tile(cid, rows)))
        for k, c in enumerate(pl.cells):
            P = 7 + int(lk.cells.lengths[c])
            x = got.chain[:, k * n_pop:(k + 1) * n_pop, :P]
            assert np.all(x >= pl.lower[k, :P]) and np.all(x <= pl.upper[k, :P])
            np.testing.assert_array_equal(got.prichain[:, k * n_pop:(k + 1) * n_pop].reshape(-1),
                                          LPO.pri(x.reshape(-1, P), pl.prior_mu[k, :P], pl.prior_sig[k, :P]))
        assert got.accept_rate.sum() > 0
        np.testing.assert_array_equal(got.pop.reshape(B, ld), got.chain[-1])
        # the reductions: the stand-alone entry points on the returned chain, group = cell
        npar = 7 + lk.cells.lengths[cid]
        group = np.repeat(np.arange(K, dtype=np.int32), n_pop)
        cr = lk.chainrhat(got.chain[2:], got.s2chain[2:], npar=npar, group=group)
        ce = lk.chainess(got.chain[2:], got.s2chain[2:], npar=npar, group=group)
        ck = lk.chainrank(got.chain[2:], got.s2chain[2:], npar=npar, group=group)
        assert got.rhat.n_rows == 5 and got.ess.n_rows == 5
        for f in ("rhat", "rhat_split", "pooled_mean", "pooled_std", "s2_rhat", "s2_pooled_std"):
            np.testing.assert_array_equal(getattr(got.rhat, f), getattr(cr, f), err_msg=f)
        for f in ("ess", "ess_split", "tau", "mcse", "window", "s2_ess"):
            np.testing.assert_array_equal(getattr(got.ess, f), getattr(ce, f), err_msg=f)
        for f in ("q", "q_tail", "rhat_bulk", "rhat_folded", "rhat_rank", "s2_rhat_rank"):
            np.testing.assert_array_equal(getattr(got.rank, f), getattr(ck, f), err_msg=f)


def test_the_sampler_targets_the_gaussian_it_is_given(lk):
    """demczs_oracle.TARGET on the device: a likelihood flat to about 1e-8 in logr and a Gaussian prior on every
    coordinate; the pooled mean and std after burn-in within TARGET_Z Monte-Carlo standard errors of mu and sig. The
    least ESS per coordinate is printed beside DE-MC's 50 to 100 at 64 members and about as many evaluations (the
    number this sampler exists to move; it is not asserted)."""
    c = CELLS[0]
    P = 7 + int(lk.cells.lengths[c])
    T = O.TARGET
    pop0, z0, lo, up, mu, sig = O.gaussian_target(P, T["n_pop"], T["m0"], T["pop_seed"])
    got = lk.demczs(pop0[None], z0[None], [c], lo, up, mu, sig, T["jitter"] * sig, sigma2_0=T["sigma2_0"], n_gen=T["n_gen"],
                    thin=T["thin"], jump_every=0, CR=T["CR"], updatesigma=False, seed=T["seed"], keys=[c],
                    append_every=T["append_every"], p_snooker=T["p_snooker"])
    z, ess = D.worst_z(got.chain[T["n_burn"] // T["thin"]:], mu, sig)
    print(f"device: worst z {z:.3f}, least ESS {ess:.1f} (DE-MC at 64 members: 50 to 100), accept "
          f"{got.accept_rate.mean():.3f}, {int(got.n_null.sum())} null, {int(got.n_oob.sum())} out of bounds, "
          f"{got.kernel_ms:.1f} ms")
    assert got.n_archive == T["m0"] + T["n_pop"] * (T["n_gen"] // T["append_every"])
    assert got.n_oob.sum() < 0.01 * T["n_pop"] * T["n_gen"]
    assert z <= O.TARGET_Z


def test_refusals_name_the_offender_and_leave_the_context_usable(lk):
    from transcriptioncycleinference_amd import TciError, _lib

    pl = plan(lk.cells, CELLS, 4, 6)

    def refused(code, *words, p=pl, **kw):
        with pytest.raises(TciError) as e:
            device(lk, p, **{"n_gen": 1, **kw})
        assert e.value.code == code
        for w in words:
            assert w in str(e.value), str(e.value)
        device(lk, pl, n_gen=1)   # a valid call on the same context succeeds

    cut = lambda **ch: dataclasses.replace(pl, **ch)  # noqa: E731
    refused(_lib.TCI_EINVAL, "m0", p=cut(z0=pl.z0[:, :2]))
    refused(_lib.TCI_EINVAL, "p_snooker", p_snooker=1.5)
    refused(_lib.TCI_EINVAL, "p_snooker", p_snooker=np.nan)
    refused(_lib.TCI_EINVAL, "append_every", append_every=0)
    refused(_lib.TCI_EINVAL, "2^24 rows", n_gen=2 ** 22, append_every=1, thin=0)
    refused(_lib.TCI_EINVAL, "CR", CR=1.5)
    refused(_lib.TCI_EINVAL, "flags", flags=1)
    out = pl.z0.copy()
    out[1, 5, 5] = 1.5    # A above its upper bound 1
    refused(_lib.TCI_EINVAL, "z0", "cell 1", "row 5", "index 5", "outside", p=cut(z0=out))
    nan = pl.z0.copy()
    nan[2, 3, 40] = np.nan
    refused(_lib.TCI_EINVAL, "z0", "cell 2", "row 3", "index 40", "not finite", p=cut(z0=nan))
    bad = pl.pop0.copy()
    bad[1, 2, 5] = 1.5
    refused(_lib.TCI_EINVAL, "pop0", "cell 1", "member 2", "index 5", "outside", p=cut(pop0=bad, z0=out))   # pop0 first
    refused(_lib.TCI_EINVAL, "thin", thin=0, rhat=True)
    refused(_lib.TCI_EINVAL, "fewer than 2 kept rows", n_gen=4, thin=2, stats_from=4, rhat=True)


def test_fit_with_demczs_pools_the_chains_and_none_is_todays_fit(lk):
    from transcriptioncycleinference_amd import mcmc

    a, b = CELLS[0], CELLS[1]
    kw = dict(cells=[a, b], n_steps=300, n_burn=1, thin=1, seed=3)
    plain, none = mcmc.fit(lk, **kw), mcmc.fit(lk, demczs=None, **kw)
    assert plain.MCMCdemczs is None and none.MCMCdemczs is None and none.MCMCdemc is None
    for x, y in zip(plain.MCMCchain, none.MCMCchain):
        for f in mcmc.CHAIN_FIELDS:
            np.testing.assert_array_equal(x[f], y[f])
    zs = dict(n_pop=3, n_gen=12, m0=20, append_every=4, p_snooker=0.5)
    fr = mcmc.fit(lk, cells=[a, b], n_burn=4, thin=2, seed=3, demczs=zs)
    res, sp = mcmc.demczs(lk, thin=2, n_burn=4, seed=3, cells=[a, b], log_rows=12, **zs)
    assert [set(e) for e in fr.MCMCdemczs] == [set(mcmc.DEMCZS_FIELDS)] * 2 and fr.MCMCdemc is None
    np.testing.assert_array_equal(res.chain[0].reshape(2, 3, -1), sp.pop0[:, :3])   # chain i starts at replicate i's x0
    np.testing.assert_array_equal(sp.pop0[:, :3], mcmc.search_population(lk.cells, [a, b], 3, 3).pop0)
    for k, c in enumerate((a, b)):
        n = int(lk.cells.lengths[c])
        e = fr.MCMCdemczs[k]
        assert e["cell_index"] == c + 1 and e["n_pop"] == 3 and e["n_gen"] == 12 and e["m0"] == 20 and e["n_archive"] == 29
        np.testing.assert_array_equal(e["accept_rate"], res.accept_rate[k])
        np.testing.assert_array_equal(e["n_null"], res.n_null[k])
        assert e["snooker_rate"] == res.snooker[:, k * 3:(k + 1) * 3].mean()
        assert e["rhat_max"] == np.nanmax(np.append(res.rhat.rhat[k, :7 + n], res.rhat.s2_rhat[k]))
        assert e["ess_min"] == np.nanmin(np.append(res.ess.ess[k, :7 + n], res.ess.s2_ess[k]))
        pooled = res.chain[2:, k * 3:(k + 1) * 3, :7 + n].reshape(-1, 7 + n)
        np.testing.assert_array_equal(fr.MCMCchain[k]["v_chain"], pooled[:, 0])
        np.testing.assert_allclose([fr.MCMCresults[k]["mean_v"], fr.MCMCresults[k]["sigma_v"]],
                                   [pooled[:, 0].mean(), pooled[:, 0].std()], rtol=1e-12)
        np.testing.assert_array_equal(fr.final_theta[k], res.pop[k, 0])
    # from a mode search's final population: the archive is the search's, the chains start at its best members
    sr = mcmc.modesearch(lk, n_pop=20, n_gen=5, seed=3, cells=[a, b])
    pre, _ = mcmc.demczs(lk, n_pop=3, m0=20, n_gen=2, seed=3, cells=[a, b], presearch=dict(n_gen=5), rhat=False, ess=False,
                         archive=True, append_every=1)
    np.testing.assert_array_equal(pre.archive[:, :20], sr[0].pop)
    for k in range(2):
        np.testing.assert_array_equal(pre.chain[0, k * 3:(k + 1) * 3], sr[0].pop[k, mcmc.search_order(sr[0].f[k])[:3]])
    shard, _ = mcmc.demczs(lk, thin=2, n_burn=4, seed=3, cells=[b], **zs)
    np.testing.assert_array_equal(shard.pop[0, :, :7 + int(lk.cells.lengths[b])], res.pop[1, :, :7 + int(lk.cells.lengths[b])])
