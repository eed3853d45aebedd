"""The DE-MC(zs) sampler's host side (no GPU): defaults, struct layouts, fit's refusals, and the numpy restatement
(tests/demczs_oracle.py) with a synthetic SS: the index draw, the butterfly sum, the archive's schedule, and the
distribution it must target, with and without the right Jacobian."""
import ctypes as C
import itertools

import numpy as np
import pytest

import demc_oracle as D
import demczs_oracle as O


@pytest.fixture(scope="module")
def lib():
    from transcriptioncycleinference_amd import _lib
    from transcriptioncycleinference_amd.build import build_library

    build_library()
    return _lib.load()


def flat_ss(rows):
    return np.ones(len(rows))


def test_defaults_and_struct_layouts(lib):
    from transcriptioncycleinference_amd import _lib

    o = _lib.tci_demczs_options()
    assert lib.tci_demczs_defaults(C.byref(o)) == _lib.TCI_OK
    assert (o.n_gen, o.thin, o.jump_every, o.stats_from, o.updatesigma, o.CR, o.gamma0, o.seed, o.flags, o.append_every,
            o.p_snooker) == (1000, 1, 10, 0, 1, 0.2, 0.0, 0, 0, 10, 0.1)
    assert not o.keys
    assert lib.tci_demczs_defaults(None) == _lib.TCI_EINVAL
    assert lib.tci_demczs_run(None, None, None, None, 0, None, 0, 0, 0, None, None, None, None, None, None, None, None, None,
                              None, None) == _lib.TCI_EINVAL
    assert C.sizeof(_lib.tci_demczs_options) == 96 and C.sizeof(_lib.tci_demczs_outputs) == 168
    names = [f for f, _ in _lib.tci_demczs_outputs._fields_]
    assert names[:16] == [f for f, _ in _lib.tci_demc_outputs._fields_]
    assert names[16:] == ["n_null", "ljac", "snooker", "archive", "n_archive"]


def test_fit_refuses_demczs_with_the_other_samplers_and_bad_keys():
    from transcriptioncycleinference_amd import mcmc

    for kw in (dict(replicates=2, rhat=False), dict(temper=2)):
        with pytest.raises(ValueError, match="temper or replicates"):
            mcmc.fit(None, demczs=dict(n_gen=4), thin=1, **kw)
    with pytest.raises(ValueError, match="two samplers"):
        mcmc.fit(None, demczs=dict(n_gen=4), demc=dict(n_gen=4), thin=1)
    with pytest.raises(ValueError, match="DRAM reductions"):
        mcmc.fit(None, demczs=dict(n_gen=4), thin=1, diagnostics=True)
    with pytest.raises(ValueError, match="unknown keys"):
        mcmc._demczs_arg(dict(n_pop=8, F=0.5))
    with pytest.raises(ValueError, match="n_pop"):
        mcmc._demczs_arg(dict(n_pop=0))
    with pytest.raises(ValueError, match="m0"):
        mcmc._demczs_arg(dict(n_pop=8, m0=7))
    assert mcmc._demczs_arg({}) == dict(n_pop=4, n_gen=1000)
    assert "MCMCdemczs" in mcmc.FitResult.__dataclass_fields__
    assert set(mcmc.DEMC_FIELDS) < set(mcmc.DEMCZS_FIELDS) and set(mcmc.DEMC_KEYS) < set(mcmc.DEMCZS_KEYS)


def test_default_archive_is_ten_rows_per_parameter_of_the_longest_cell(cells):
    from transcriptioncycleinference_amd import mcmc

    assert mcmc.demczs_m0(cells, [290, 0, 219]) == 10 * 136 and mcmc.demczs_m0(cells, [290]) == 1200


@pytest.mark.parametrize("M", [3, 4, 5, 7])
def test_index_rule_gives_three_distinct_rows_each_uniform_over_its_range(M):
    """The scaling rule by exhaustion: m(w, n) takes every value of [0, n) on words spread over [0, 2^32), so running
    the rule over every (m(w.x), m(w.y), m(w.w)) triple, one word per value, enumerates its whole image. Every ordered
    triple of distinct rows appears exactly once: a is uniform over M rows, c over the M - 1 others, e over the M - 2
    left."""
    word = lambda v, n: -(-(v << 32) // n)   # noqa: E731  the least word that scales to v
    for n in (M, M - 1, M - 2):
        assert [int(O.scale(word(v, n), n)) for v in range(n)] == list(range(n))
        assert int(O.scale(2 ** 32 - 1, n)) == n - 1
    seen = [O.scale_rule(word(i, M), word(j, M - 1), word(k, M - 2), M)
            for i in range(M) for j in range(M - 1) for k in range(M - 2)]
    assert all(len({a, c, e}) == 3 and 0 <= min(a, c, e) and max(a, c, e) < M for a, c, e in seen)
    assert sorted(seen) == sorted(itertools.permutations(range(M), 3))


def test_index_draws_at_once_are_the_scalar_ones_and_stay_in_range():
    for M in (3, 7, 1300, 2 ** 24 - 1):
        a, c, e, jr, snk, gs = O.index_draws(7, 3, 5, 70, M, 120, 0.5)
        for i in (0, 1, 33, 69):
            assert (a[i], c[i], e[i], jr[i], snk[i], gs[i]) == O.index_draw(7, 3, 5, i, M, 120, 0.5)
        assert np.all((a != c) & (a != e) & (c != e)) and max(a.max(), c.max(), e.max()) < M and jr.max() < 120
        assert np.all((gs > 1.2) & (gs < 2.2)) and 0 < snk.sum() < 70


def test_butterfly_sum_is_the_six_fold_numpy_fold():
    x = np.random.default_rng(1).normal(size=(5, 2055)) * 10.0 ** np.random.default_rng(2).integers(-8, 8, (5, 2055))
    for P in (1, 12, 63, 64, 65, 120, 136, 2055):
        want = [O.sum64_loops(r[:P]) for r in x]
        np.testing.assert_array_equal(O.sum64(x[:, :P]), want)
        assert O.sum64(x[0, :P]) == want[0]
    # the order matters: the plain ascending sum differs somewhere
    assert any(O.sum64(r) != np.add.reduce(r) or O.sum64(r) != sum(r.tolist()) for r in x)


def test_butterfly_sum_at_the_lane_edges_and_the_longest_row():
    """The shapes of tests/test_demczs_shapes_gpu.py: n = 9 (lanes 9 to 63 add nothing), 64 and 128 (every trip full), 65
    and 129 (the last trip holds lane 0 alone) and 2055 (33 terms in lanes 0 to 6, 32 in the others). Terms of mixed sign
    over 16 decades, so that the association order decides the low bits."""
    rs = np.random.default_rng(4)
    x = rs.normal(size=(6, 2056)) * 10.0 ** rs.integers(-8, 8, (6, 2056))
    assert np.all((x > 0).any(axis=1) & (x < 0).any(axis=1))
    differs = 0
    for n in (9, 64, 65, 128, 129, 2055):
        want = [O.sum64_loops(r[:n]) for r in x]
        np.testing.assert_array_equal(O.sum64(x[:, :n]), want)
        assert all(O.sum64(r[:n]) == w for r, w in zip(x, want))
        differs += sum(w != sum(r[:n].tolist()) for r, w in zip(x, want))
        # one term more or fewer in the last trip changes the sum: the count is not rounded to a trip
        assert any(O.sum64(r[:n]) != O.sum64(r[:n - 1]) for r in x) and any(O.sum64(r[:n]) != O.sum64(r[:n + 1]) for r in x)
    assert differs > 0      # the plain ascending sum is another order


@pytest.mark.parametrize("M", [2 ** 16 + 5, 2 ** 24 - 1])
def test_index_rule_at_archives_past_2_16_rows(M):
    """m(w, n) = floor(w n / 2^32) in Python integers, where the product needs up to 56 bits, on the words 0, 2^32 - 1 and
    some between: three distinct rows in range from scale_rule, and the same rows from index_draws' uint64 arithmetic on
    the generator's words."""
    words = (0, 1, 2 ** 16 - 1, 2 ** 16, 0x7FFFFFFF, 0x80000000, 0xFFFF0000, 2 ** 32 - 2, 2 ** 32 - 1)
    m = lambda w, n: w * n // 2 ** 32   # noqa: E731

    def rule(wx, wy, ww):
        a, c, e = m(wx, M), m(wy, M - 1), m(ww, M - 2)
        c += c >= a
        e += e >= min(a, c)
        e += e >= max(a, c)
        return a, c, e

    assert m(2 ** 32 - 1, M) == M - 1 and m(2 ** 32 - 1, M - 2) == M - 3 and m(0, M) == 0
    assert m(2 ** 16, M) == M >> 16 and m(0x80000000, M) == M >> 1      # a 32-bit product would lose these
    top = 0
    for wx, wy, ww in itertools.product(words, repeat=3):
        a, c, e = got = O.scale_rule(wx, wy, ww, M)
        assert got == rule(wx, wy, ww) and len({a, c, e}) == 3 and 0 <= min(got) and max(got) < M
        top = max(top, *got)
    assert top == M - 1 and O.scale_rule(0, 0, 0, M) == (0, 1, 2)
    assert O.scale_rule(2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1, M) == (M - 1, M - 2, M - 3)
    n_pop, P = 4096, 9
    a, c, e, jr, _, _ = O.index_draws(7, 3, 5, n_pop, M, P, 0.5)
    w = D.rng_vec(7, 3, 5, O.P_INDEX, np.arange(n_pop))
    want = [rule(int(w[0][i]), int(w[1][i]), int(w[3][i])) for i in range(n_pop)]
    np.testing.assert_array_equal(np.stack([a, c, e], axis=1), np.array(want, np.int64))
    assert [int(v) for v in jr] == [m(int(v), P) for v in w[2]]
    assert max(a.max(), c.max(), e.max()) >= M - M // 256 and a.dtype == np.int64   # 12,288 draws reach the top 1/256


def test_the_parallel_move_at_once_is_demc_oracles_trial():
    rs = np.random.default_rng(3)
    P, ld, n = 120, 125, 6
    x, x1, x2 = (rs.normal(size=(n, ld)) for _ in range(3))
    lo, up, jit = np.full(ld, -4.0), np.full(ld, 4.0), np.full(ld, 0.01)
    ii, jr = np.array([0, 3, 4, 9, 70, 4095]), rs.integers(0, P, n)
    seen = set()
    for jump in (False, True):
        t, ob = O.parallel(x, x1, x2, ii, jr, 7, 3, 5, P, lo, up, jit, 0.3, 2.38, jump)
        for r in range(n):
            u, v = O.coord_uniforms(7, 3, 5, int(ii[r]), P)
            tr, obr, _ = D.trial(np.stack([x[r], x1[r], x2[r]]), 0, 1, 2, int(jr[r]), u, v, P, lo, up, jit, 0.3, 2.38, jump)
            np.testing.assert_array_equal(t[r], tr)
            assert ob[r] == obr
            seen.add(bool(obr))
    assert seen == {False, True}


def small_run(jac_dim=None, **kw):
    T = {**O.SMALL, **kw}
    P = T["P"]
    pop0, z0, lo, up, mu, sig = O.gaussian_target(P, T["n_pop"], T["m0"], T["pop_seed"])
    r = O.run(flat_ss, pop0, z0, P, lo, up, mu, sig, T["jitter"] * sig, sigma2_0=T["sigma2_0"], key=290, seed=T["seed"],
              n_gen=T["n_gen"], thin=T["thin"], jump_every=0, CR=T["CR"], append_every=T["append_every"],
              p_snooker=T["p_snooker"], jac_dim=jac_dim)
    return r, T, mu, sig, z0


def test_archive_grows_by_the_stated_schedule():
    assert [O.archive_rows(g, 7, 3, 2) for g in range(1, 8)] == [7, 7, 10, 10, 13, 13, 16]
    assert [O.archive_rows(g, 3, 5, 1) for g in range(1, 4)] == [3, 8, 13]
    r, T, _, _, z0 = small_run(n_pop=3, m0=7, n_gen=7, thin=1, append_every=2)
    Z = r["archive"]
    assert Z.shape[0] == 7 + 3 * 3
    np.testing.assert_array_equal(Z[:7], z0)
    for q, g in enumerate((2, 4, 6)):
        np.testing.assert_array_equal(Z[7 + 3 * q:10 + 3 * q], r["chain"][g])
    # a null move: a chain that has not moved since it was archived and draws its own copy has D = 0
    x = z0[0]
    t, flag, lj, D, _ = O.snooker(x, x.copy(), z0[1], z0[2], 1.7, 12, np.full(12, -np.inf), np.full(12, np.inf))
    assert flag == 2 and D == 0 and np.isnan(lj) and np.array_equal(t, x)


def test_restatement_recovers_a_small_gaussian_and_a_wrong_jacobian_does_not():
    """O.SMALL: P = 12, every other move a snooker move. With the exponent (P - 1) / 2 the pooled mean and std of every
    coordinate are within TARGET_Z standard errors; with P / 2 in its place the standard deviations come out about
    3.5 % wide and the same bound refuses the run. Measured on these runs (seed 3): worst |z| 1.79 and 7.11, least ESS
    about 13,500 either way."""
    for jac_dim, ok in ((None, True), (O.SMALL["P"], False)):
        r, T, mu, sig, _ = small_run(jac_dim)
        z, ess = D.worst_z(r["chain"][T["n_burn"] // T["thin"]:], mu, sig)
        print(f"exponent {jac_dim or T['P'] - 1}/2: worst z {z:.3f}, least ESS {ess:.1f}, accept {r['accept_rate'].mean():.3f}, "
              f"{int(r['n_null'].sum())} null, {int(r['n_oob'].sum())} out of bounds")
        assert r["snooker"].mean() == pytest.approx(0.5, abs=0.01) and r["n_null"].sum() > 0
        assert (z <= O.TARGET_Z) == ok, (jac_dim, z)


def test_restatement_targets_the_gaussian_it_is_given():
    """O.TARGET on the restatement with a constant SS: P = 120, 4 chains, 1,200 archive rows. Measured on this run
    (seed 3, 20,000 generations, every 10th kept, the first 5,000 dropped): worst |z| 2.57 over the 240 statistics,
    least ESS 25, acceptance 0.27; TARGET_Z = 5 leaves the margin of 2 the sizing asked for."""
    T = O.TARGET
    P = 120
    pop0, z0, lo, up, mu, sig = O.gaussian_target(P, T["n_pop"], T["m0"], T["pop_seed"])
    r = O.run(flat_ss, pop0, z0, P, lo, up, mu, sig, T["jitter"] * sig, sigma2_0=T["sigma2_0"], key=290, seed=T["seed"],
              n_gen=T["n_gen"], thin=T["thin"], jump_every=0, CR=T["CR"], append_every=T["append_every"],
              p_snooker=T["p_snooker"])
    assert not r["undecided"]
    z, ess = D.worst_z(r["chain"][T["n_burn"] // T["thin"]:, :, :P], mu, sig)
    print(f"restatement: worst z {z:.3f}, least ESS {ess:.1f}, accept {r['accept_rate'].mean():.3f}")
    assert r["archive"].shape[0] == T["m0"] + T["n_pop"] * (T["n_gen"] // T["append_every"])
    assert 0.1 < r["accept_rate"].mean() < 0.5
    assert z <= O.TARGET_Z - 2
