"""The mode search on the device (tci_modesearch / tci_modesearch.hip) against the numpy restatement
(tests/modesearch_oracle.py). The restatement takes Likelihood.ss_batch as its SS function, the same kernel and hence
the same bits, so every output is compared bit for bit; ss_best and f_best are also held against the C oracle at
theta_best within the project's parity tolerance."""
import numpy as np
import pytest

import modesearch_oracle as O
import ragged_cases as RC

pytestmark = pytest.mark.gpu

CELLS = (290, 0, 219)        # TestData cells of 113, 120 and 129 points
SEED = 11
PARITY = 1e-10
FIELDS = ("pop", "f", "ss", "best", "theta_best", "f_best", "ss_best", "pri_best", "f_trace", "n_accepted")


@pytest.fixture(scope="module")
def lk(cells):
    from transcriptioncycleinference_amd import Likelihood

    assert tuple(int(cells.lengths[c]) for c in CELLS) == (113, 120, 129)
    with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as L:
        yield L


def population(cl, ids, n_pop, v0=None):
    from transcriptioncycleinference_amd import mcmc

    return mcmc.search_population(cl, ids, SEED, n_pop, v0=v0)


def oracle_cell(lk, sp, k, key, **kw):
    c = sp.cells[k]
    P = 7 + int(lk.cells.lengths[c])
    return O.search(lambda rows: lk.ss_batch(rows, np.full(len(rows), c, np.int32)), sp.pop0[k], P, sp.lower[k],
                    sp.upper[k], sp.prior_mu[k], sp.prior_sig[k], key=key, seed=SEED, **kw)


def device(lk, sp, **kw):
    return lk.modesearch(sp.pop0, np.array(sp.cells, np.int32), sp.lower, sp.upper, sp.prior_mu, sp.prior_sig, seed=SEED,
                         **kw)


def assert_cell(got, k, want, n_gen):
    for f in FIELDS:
        g = getattr(got, f)
        g = g[:, k] if f in ("f_trace", "n_accepted") else g[k]
        w = np.asarray(want[f])
        np.testing.assert_array_equal(np.asarray(g), w.reshape(np.shape(g)), err_msg=f"{f} of cell {k}")
    assert got.f_trace.shape[0] == n_gen + 1 and got.n_accepted.shape[0] == n_gen


@pytest.mark.parametrize("n_pop", [4, 8, 70])
@pytest.mark.parametrize("CR", [0.0, 0.9, 1.0])
def test_replay_bit_for_bit(lk, n_pop, CR):
    sp = population(lk.cells, CELLS, n_pop)
    got = device(lk, sp, n_gen=3, CR=CR)
    assert got.n_evals == 3 * n_pop * 4
    for k in range(3):
        assert_cell(got, k, oracle_cell(lk, sp, k, key=k, n_gen=3, CR=CR), 3)
    if CR > 0:
        assert got.n_accepted.sum() > 0   # the replay is of a search that moves
    assert np.all(np.diff(got.f_trace, axis=0) <= 0)


def test_generation_zero_is_the_objective_of_pop0(lk):
    import chainlp_oracle as LPO

    sp = population(lk.cells, CELLS, 8)
    s2 = np.array([1.0, 2.5, 0.125])
    got = device(lk, sp, n_gen=0, s2=s2)
    for k, c in enumerate(CELLS):
        P = 7 + int(lk.cells.lengths[c])
        ss = lk.ss_batch(sp.pop0[k], np.full(8, c, np.int32))
        f = ss / s2[k] + LPO.pri(sp.pop0[k][:, :P], sp.prior_mu[k, :P], sp.prior_sig[k, :P])
        np.testing.assert_array_equal(got.ss[k], ss)
        np.testing.assert_array_equal(got.f[k], f)
        np.testing.assert_array_equal(got.pop[k], sp.pop0[k])
        assert got.best[k] == int(np.argmin(f)) and got.f_trace[0, k] == f.min()
    assert got.n_accepted.shape == (0, 3)


def test_a_cell_does_not_depend_on_its_neighbours_position_or_ld(lk):
    from transcriptioncycleinference_amd import mcmc

    sp = population(lk.cells, CELLS, 8)
    together = device(lk, sp, n_gen=3)
    c, k = CELLS[0], 0
    # cell c alone behind another cell, with five more columns of padding, keyed as it was in the three-cell call
    two = population(lk.cells, (CELLS[2], c), 8)
    ld = two.pop0.shape[2] + 5
    wide = lambda a, fill: np.concatenate([a, np.full(a.shape[:-1] + (ld - a.shape[-1],), fill)], axis=-1)  # noqa: E731
    sp2 = mcmc.SearchPlan(two.cells, wide(two.pop0, 7.0), wide(two.lower, -np.inf), wide(two.upper, np.inf),
                          wide(two.prior_mu, 0.0), wide(two.prior_sig, np.inf))
    np.testing.assert_array_equal(sp2.pop0[1, :, :sp.pop0.shape[2]], sp.pop0[k])
    alone = device(lk, sp2, n_gen=3, keys=[5, k])
    P = 7 + int(lk.cells.lengths[c])
    for f in FIELDS:
        a, b = getattr(alone, f), getattr(together, f)
        a, b = (a[:, 1], b[:, k]) if f in ("f_trace", "n_accepted") else (a[1], b[k])
        if f in ("pop", "theta_best"):
            a, b = a[..., :P], b[..., :P]
        np.testing.assert_array_equal(a, b, err_msg=f)
    assert np.all(alone.pop[1, :, two.pop0.shape[2]:] == 7.0) and np.all(np.isnan(alone.theta_best[1, P:]))   # padding: the parent's
    # another key is another search; the key itself reproduces it
    one = population(lk.cells, (c,), 8)
    other = device(lk, one, n_gen=3, keys=[9])
    assert not np.array_equal(other.pop[0], together.pop[k, :, :P])
    again = device(lk, one, n_gen=3, keys=[k])
    np.testing.assert_array_equal(again.pop[0], together.pop[k, :, :P])   # ld = P here, 136 there
    np.testing.assert_array_equal(again.f[0], together.f[k])


def test_best_member_agrees_with_the_c_oracle(lk, c_oracle, construct):
    cl = lk.cells
    sp = population(cl, CELLS, 8)
    got = device(lk, sp, n_gen=3)
    theta = np.where(np.isnan(got.theta_best), 0.0, got.theta_best)
    want, st = c_oracle.ss_batch(cl.offsets, cl.t, cl.ms2, cl.pp7, construct, theta, np.array(CELLS, np.int32))
    assert np.all(st == 0)
    for k in range(3):
        print(f"cell {CELLS[k]}: ss_best {got.ss_best[k]!r} oracle {want[k]!r}")
    np.testing.assert_allclose(got.ss_best, want, rtol=PARITY, atol=0)
    np.testing.assert_allclose(got.f_best, want / 1.0 + got.pri_best, rtol=PARITY, atol=0)


def test_every_member_stays_inside_its_bounds(lk):
    sp = population(lk.cells, CELLS, 8)
    v0 = {CELLS[1] + 1: 4.2}   # a hierarchical cell: v within 1e-5 of 4.2
    hier = population(lk.cells, (CELLS[1],), 8, v0=v0)
    assert hier.lower[0, 0] == 4.2 - 1e-5 and hier.upper[0, 0] == 4.2 + 1e-5
    for plan in (sp, hier):
        got = device(lk, plan, n_gen=5, F=1.5)   # a long step: mutants leave the box and are refused
        for k, c in enumerate(plan.cells):
            P = 7 + int(lk.cells.lengths[c])
            x = got.pop[k, :, :P]
            assert np.all(x >= plan.lower[k, :P]) and np.all(x <= plan.upper[k, :P])


def test_long_cell_replays_bit_for_bit():
    from transcriptioncycleinference_amd import Likelihood, from_lists

    cl = from_lists(RC.context_cells("tile")[0])
    c = int(np.argmax(cl.lengths))
    assert cl.lengths[c] == 600    # P = 607: past the 520 of the register-resident kernels
    with Likelihood(cl, "P2P-MS2v5-LacZ-PP7v4", device=0) as L:
        assert L.info["rows_per_lane"] == 0
        sp = population(cl, (c,), 4)
        got = device(L, sp, n_gen=2)
        assert_cell(got, 0, oracle_cell(L, sp, 0, key=0, n_gen=2), 2)


def test_refusals_name_the_offender_and_leave_the_context_usable(lk):
    from transcriptioncycleinference_amd import TciError, _lib, mcmc

    sp = population(lk.cells, CELLS, 4)

    def refused(code, *words, plan=sp, **kw):
        with pytest.raises(TciError) as e:
            device(lk, plan, n_gen=1, **kw)
        assert e.value.code == code
        for w in words:
            assert w in str(e.value), str(e.value)
        device(lk, sp, n_gen=1)   # a valid call on the same context succeeds

    cut = lambda p, **ch: mcmc.SearchPlan(**{**p.__dict__, **ch})  # noqa: E731
    refused(_lib.TCI_EINVAL, "n_pop", plan=cut(sp, pop0=sp.pop0[:, :3]))
    out = sp.pop0.copy()
    out[1, 2, 5] = 1.5    # A above its upper bound 1
    refused(_lib.TCI_EINVAL, "cell 1", "member 2", "index 5", "outside", plan=cut(sp, pop0=out))
    nan = sp.pop0.copy()
    nan[2, 3, 40] = np.nan
    refused(_lib.TCI_EINVAL, "cell 2", "member 3", "index 40", "not finite", plan=cut(sp, pop0=nan))
    refused(_lib.TCI_EINVAL, "F", F=0.0)
    refused(_lib.TCI_EINVAL, "CR", CR=1.5)
    refused(_lib.TCI_EINVAL, "flags", flags=1)
    short = 7 + 120   # long enough for the first two cells, one short of nothing for the third (P = 136)
    refused(_lib.TCI_ERANGE, "cell 2", "136", plan=cut(sp, pop0=sp.pop0[:, :, :short], lower=sp.lower[:, :short],
                                                         upper=sp.upper[:, :short], prior_mu=sp.prior_mu[:, :short],
                                                         prior_sig=sp.prior_sig[:, :short]))


def test_presearch_fit_starts_from_the_search_and_none_is_todays_fit(lk):
    from transcriptioncycleinference_amd import mcmc

    a, b = CELLS[0], CELLS[1]
    kw = dict(cells=[a, b], n_steps=300, n_burn=1, thin=1, replicates=2, seed=3)
    plain = mcmc.fit(lk, **kw)
    none = mcmc.fit(lk, presearch=None, **kw)
    assert none.MCMCsearch is None and plain.MCMCsearch is None
    for x, y in zip(plain.MCMCchain, none.MCMCchain):
        for f in mcmc.CHAIN_FIELDS:
            np.testing.assert_array_equal(x[f], y[f])
    np.testing.assert_array_equal(plain.final_theta, none.final_theta)
    pre = mcmc.fit(lk, presearch=dict(n_pop=8, n_gen=5), **kw)
    assert [set(e) for e in pre.MCMCsearch] == [set(mcmc.SEARCH_FIELDS)] * 2
    for k, c in enumerate((a, b)):
        e, ch = pre.MCMCsearch[k], pre.MCMCchain[k]
        n = int(lk.cells.lengths[c])
        row0 = mcmc.chain_theta(ch, n, np.array([0]))[0]
        np.testing.assert_array_equal(row0, e["theta_best"])
        assert e["cell_index"] == c + 1 and e["n_pop"] == 8 and e["n_gen"] == 5 and e["n_evals"] == 48
        assert e["f_best"] <= e["f0_best"] == e["f_trace"][0] and e["f_best"] == e["f_trace"][-1]
    # the search the fit ran is mcmc.modesearch's with the fit's seed
    sr, _ = mcmc.modesearch(lk, n_pop=8, n_gen=5, seed=3, cells=[a, b])
    np.testing.assert_array_equal(sr.f_best, [e["f_best"] for e in pre.MCMCsearch])


def test_presearch_starts_replicate_r_from_the_r_th_best_member_and_rungs_from_their_replicates(lk):
    from transcriptioncycleinference_amd import mcmc

    ids = [CELLS[0], CELLS[1]]
    K, M, R = 2, 2, 2
    sr, _ = mcmc.modesearch(lk, n_pop=8, n_gen=5, seed=3, cells=ids)
    # dram_run's own first kept row is the start: the fit's chain rows come through a spy on dram_run
    seen = {}
    real = mcmc.dram_run

    def spy(lk_, cell_id, theta0, *a, **k):
        seen["cell_id"], seen["theta0"] = np.array(cell_id), np.array(theta0)
        return real(lk_, cell_id, theta0, *a, **k)

    mcmc.dram_run = spy
    try:
        fr = mcmc.fit(lk, cells=ids, n_steps=300, n_burn=1, thin=1, replicates=M, temper=R, seed=3,
                      presearch=dict(n_pop=8, n_gen=5))
    finally:
        mcmc.dram_run = real
    assert seen["theta0"].shape[0] == M * R * K
    for k, c in enumerate(ids):
        P = 7 + int(lk.cells.lengths[c])
        order = mcmc.search_order(sr.f[k])
        assert order[0] == sr.best[k] and sr.f[k, order[0]] <= sr.f[k, order[1]]
        assert not np.array_equal(sr.pop[k, order[0], :P], sr.pop[k, order[1], :P])
        for q in range(R):
            for r in range(M):
                row = (q * M + r) * K + k
                assert seen["cell_id"][row] == c
                np.testing.assert_array_equal(seen["theta0"][row, :P], sr.pop[k, order[r], :P],
                                              err_msg=f"cell {k}, replicate {r}, rung {q}")
        # and the cold rung of replicate 0 is what the run's first chain row holds
        np.testing.assert_array_equal(mcmc.chain_theta(fr.MCMCchain[k], P - 7, np.array([0]))[0],
                                      fr.MCMCsearch[k]["theta_best"])
    # the untempered replicate fit: replicate 1's chain itself starts from the second best member
    seen.clear()
    mcmc.dram_run = spy
    try:
        mcmc.fit(lk, cells=ids, n_steps=300, n_burn=1, thin=1, replicates=M, seed=3, presearch=dict(n_pop=8, n_gen=5))
    finally:
        mcmc.dram_run = real
    for k, c in enumerate(ids):
        P = 7 + int(lk.cells.lengths[c])
        order = mcmc.search_order(sr.f[k])
        np.testing.assert_array_equal(seen["theta0"][1 * K + k, :P], sr.pop[k, order[1], :P])
