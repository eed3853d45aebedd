"""The DE-MC sampler's host side (no GPU): defaults, the checks that need no device, fit's refusals, and the numpy
restatement (tests/demc_oracle.py) against the distribution it must target, with the C oracle as its SS function."""
import ctypes as C

import numpy as np
import pytest

import demc_oracle as O


@pytest.fixture(scope="module")
def lib():
    from transcriptioncycleinference_amd import _lib
    from transcriptioncycleinference_amd.build import build_library

    build_library()
    return _lib.load()


def test_defaults_are_the_documented_ones(lib):
    from transcriptioncycleinference_amd import _lib

    o = _lib.tci_demc_options()
    assert lib.tci_demc_defaults(C.byref(o)) == _lib.TCI_OK
    assert (o.n_gen, o.thin, o.jump_every, o.stats_from, o.updatesigma, o.CR, o.gamma0, o.seed, o.flags) == \
        (1000, 1, 10, 0, 1, 0.2, 0.0, 0, 0)
    assert not o.keys
    assert lib.tci_demc_defaults(None) == _lib.TCI_EINVAL
    assert lib.tci_demc_run(None, None, None, 0, None, 0, 0, None, None, None, None, None, None, None, None, None, None,
                            None) == _lib.TCI_EINVAL


def test_struct_layouts_match_the_header():
    from transcriptioncycleinference_amd import _lib

    assert C.sizeof(_lib.tci_demc_options) == 80 and C.sizeof(_lib.tci_demc_outputs) == 128
    assert [f for f, _ in _lib.tci_demc_outputs._fields_][:4] == ["chain", "s2chain", "sschain", "prichain"]


def test_fit_refuses_demc_with_temper_replicates_and_bad_keys():
    from transcriptioncycleinference_amd import mcmc

    for kw in (dict(replicates=2, rhat=False), dict(temper=2)):
        with pytest.raises(ValueError, match="temper or replicates"):
            mcmc.fit(None, demc=dict(n_pop=8, n_gen=4), thin=1, **kw)
    with pytest.raises(ValueError, match="DRAM reductions"):
        mcmc.fit(None, demc=dict(n_pop=8, n_gen=4), thin=1, diagnostics=True)
    with pytest.raises(ValueError, match="unknown keys"):
        mcmc._demc_arg(dict(n_pop=8, F=0.5))
    with pytest.raises(ValueError, match="n_pop"):
        mcmc._demc_arg(dict(n_pop=3))
    assert mcmc._demc_arg({}) == dict(n_pop=64, n_gen=1000)
    assert "MCMCdemc" in mcmc.FitResult.__dataclass_fields__


def test_default_jitter_is_a_thousandth_of_the_proposal_scale(cells):
    from transcriptioncycleinference_amd import mcmc

    jit = mcmc.demc_jitter(cells, [290, 0])
    plan = mcmc.plan_fit(cells, [290, 0], 0)
    P = 7 + int(cells.lengths[290])
    np.testing.assert_array_equal(jit[0, :P], 1e-3 * np.sqrt(plan.qcov_diag[0, :P]))
    assert np.all(jit[0, P:] == 0) and np.all(jit[1] > 0)


def test_index_draw_takes_two_distinct_resting_members():
    for n_pop in (4, 5, 70):
        for h in (0, 1):
            for i in range(h, n_pop, 2):
                r1, r2, jr = O.index_draw(7, 3, 2 * 5 + h, i, h, n_pop, 120)
                assert r1 != r2 and r1 % 2 != h and r2 % 2 != h and 0 <= r1 < n_pop and 0 <= r2 < n_pop and 0 <= jr < 120


@pytest.mark.parametrize("n_pop", [4, 5, 2049, 4095, 4096])
def test_index_draw_at_the_largest_populations(n_pop):
    """Every moving member of both half-sweeps, up to the 4,096 members the host admits: an odd population moves
    (n_pop + 1) / 2 members in half-sweep 0 and n_pop / 2 in half-sweep 1, and the pair comes from the other half."""
    P = 2055
    for h in (0, 1):
        movers = range(h, n_pop, 2)
        assert len(movers) == (n_pop - h + 1) // 2
        seen = set()
        for i in movers:
            r1, r2, jr = O.index_draw(7, 3, 2 * 5 + h, i, h, n_pop, P)
            assert r1 != r2 and r1 % 2 != h and r2 % 2 != h and 0 <= r1 < n_pop and 0 <= r2 < n_pop and 0 <= jr < P
            seen.add((r1, r2))
        assert len(seen) > 1 or n_pop < 6    # 4 or 5 members: two resting ones, so two ordered pairs in all


def test_coordinate_counters_are_one_per_member_and_coordinate():
    """The counter i * 4096 + j of the last member of the largest population on the longest row stays below 2^24, no
    two (i, j) share one, and coord_uniforms reads exactly that counter."""
    P = 2055
    ctr = np.arange(4096, dtype=np.int64)[:, None] * 4096 + np.arange(P, dtype=np.int64)[None, :]
    assert ctr[4095].max() == 4095 * 4096 + P - 1 < 2 ** 24
    assert len(np.unique(ctr)) == ctr.size
    u, v = O.coord_uniforms(7, 3, 11, 4095, P)
    assert u.shape == v.shape == (P,) and np.all((u > 0) & (u < 1) & (v > 0) & (v < 1))
    assert len(np.unique(np.concatenate([u, v]))) == 2 * P
    for j in (0, 63, 64, 2047, 2048, P - 1):
        w = O.rng(7, 3, 11, O.P_COORD, int(ctr[4095, j]))
        assert u[j] == O.u01(w[0], w[1]) and v[j] == O.u01(w[2], w[3])


def test_vector_philox_is_the_scalar_one():
    q = O.rng_vec(2 ** 40 + 5, 2 ** 33 + 9, 13, O.P_COORD, 3 * 4096 + np.arange(5))
    for j in range(5):
        assert tuple(int(w[j]) for w in q) == O.rng(2 ** 40 + 5, 2 ** 33 + 9, 13, O.P_COORD, 3 * 4096 + j)


def test_restatement_targets_the_gaussian_it_is_given(cells, c_oracle, construct):
    """The restatement with the C oracle's SS at sigma2 = 1e12 (a likelihood flat to about 1e-8 in logr) and a Gaussian
    prior on every coordinate: the pooled mean and std of the kept rows match mu and sig. Measured on this run (seed 3,
    64 members, 600 generations, burn-in 100, CR 0.1): worst |z| 2.33 over the 240 statistics, least ESS 51; TARGET_Z = 5
    leaves the margin of 2 the sizing asked for."""
    c = 290
    P = 7 + int(cells.lengths[c])
    assert P == 120
    T = O.TARGET
    pop0, lo, up, mu, sig = O.gaussian_target(P, T["n_pop"], T["pop_seed"])

    def ss(rows):
        out, st = c_oracle.ss_batch(cells.offsets, cells.t, cells.ms2, cells.pp7, construct, np.ascontiguousarray(rows),
                                    np.full(len(rows), c, np.int32))
        assert np.all(st == 0)
        return out

    r = O.run(ss, pop0, P, lo, up, mu, sig, T["jitter"] * sig, sigma2_0=T["sigma2_0"], key=c, seed=T["seed"],
              n_gen=T["n_gen"], thin=1, jump_every=0, CR=T["CR"])
    assert not r["undecided"]
    z, ess = O.worst_z(r["chain"][T["n_burn"]:, :, :P], mu, sig)
    print(f"restatement: worst z {z:.3f}, least ESS {ess:.1f}, accept {r['accept_rate'].mean():.3f}")
    assert 0.1 < r["accept_rate"].mean() < 0.5
    assert z <= O.TARGET_Z / 2
