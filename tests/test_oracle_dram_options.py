"""The option-space cases of tests/test_dram_options_gpu.py are not vacuous -- CPU only.

Every condition here is one on the CPU restatement's output alone (oracle/tci_dram_oracle.c), on the cells,
inputs and options of tests/dram_option_cases.py that the GPU test runs: each case reaches the branch of
run_chain it is named for, so that the GPU run compared with it is driven through the same branch of
k_accept1 / k_accept2, k_chain, k_walk, k_adapt_mfma and k_adapt_gt."""
import dataclasses

import numpy as np
import pytest

import dram_option_cases as D

GROUPS = sorted(D.GROUPS)


def _rows(case, k):
    return case.want["chain"][:, k, :7 + int(case.n[k])]


def _R(case, k, want=None):
    P = 7 + int(case.n[k])
    return (case.want if want is None else want)["R"][k, :P, :P]


def _R0(case, k):
    return np.diag(np.sqrt(case.qcov_diag[k, :7 + int(case.n[k])]))


def _chains(case):
    return range(len(case.n))


@pytest.mark.parametrize("group", GROUPS)
def test_groups_hold_the_lengths_they_are_named_for(c_oracle, group):
    cells, _ = D.group_cells(group, c_oracle)
    n_cells, n_points, _ = D.GROUPS[group]
    assert sorted(cells.lengths.tolist()) == sorted(n_cells * list(n_points))
    assert 7 + int(cells.lengths.max()) == D.GROUP_EXPECT[group][0]
    assert not np.all(np.isnan(cells.ms2)) and np.isnan(cells.ms2).any()  # NaN-masked data, not all-NaN cells


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("name", [c for c in D.CASES if c != "frozen"])
def test_every_chain_of_a_case_moves_and_stays_in_its_box(c_oracle, group, name):
    case = D.build(group, name, c_oracle)
    for k in _chains(case):
        rows, P = _rows(case, k), 7 + int(case.n[k])
        assert D.moved_mask(rows).sum() >= 10, (k, D.moved_mask(rows).sum())
        assert np.all(rows >= case.lower[k, :P]) and np.all(rows <= case.upper[k, :P])
        assert case.want["n_evals"][k] > 1


@pytest.mark.parametrize("group", GROUPS)
def test_am_never_enters_stage_2(c_oracle, group):
    case = D.build(group, "am", c_oracle)
    assert case.opts.ntry == 1
    assert not case.want["dr_counts"].any()
    # one evaluation per in-bounds stage 1 and the initial one: never more than a row each
    assert np.all(case.want["n_evals"] <= case.opts.n_steps)
    base = D.build(group, "baseline", c_oracle)
    assert base.want["dr_counts"][:, :3].sum() > 0 and np.any(base.want["n_evals"] > base.opts.n_steps)


@pytest.mark.parametrize("group", GROUPS)
def test_fixed_sigma_keeps_each_chains_own_sigma2(c_oracle, group):
    case = D.build(group, "fixed_sigma", c_oracle)
    s20 = np.asarray(case.sigma2_0)
    assert not np.any(s20 == 1.0) and len(set(s20.tolist())) == min(len(s20), len(D.FIXED_SIGMA2))
    np.testing.assert_array_equal(case.want["s2chain"], np.broadcast_to(s20, case.want["s2chain"].shape))
    np.testing.assert_array_equal(case.want["sigma_std"], 0.0)
    # and sigma2 matters: the chains differ from the baseline's fixed at 1
    base = case.run_restatement(c_oracle, sigma2_0=1.0)
    assert any(not np.array_equal(D.moved_mask(_rows(case, k)), D.moved_mask(base["chain"][:, k, :7 + int(case.n[k])]))
               for k in _chains(case))


@pytest.mark.parametrize("group", GROUPS)
def test_burnin_scales_both_ways_between_the_cases(c_oracle, group):
    """burnin_up: every chain has a burn-in window with a rejection rate below 0.05 (R * burnin_scale) and
    ends on another R than the baseline; the baseline and scales: some chain has one above 0.95."""
    up, base, scales = (D.build(group, name, c_oracle) for name in ("burnin_up", "baseline", "scales"))
    nb = D.burnin_windows(up)
    assert nb >= 3
    for k in _chains(up):
        assert D.window_rejection_rates(up, k)[:nb].min() < 0.05, k
        assert not np.allclose(_R(up, k), _R(base, k), rtol=1e-3, atol=0)
    for case in (base, scales):
        nb = D.burnin_windows(case)
        assert nb == 2
        assert max(D.window_rejection_rates(case, k)[:nb].max() for k in _chains(case)) > 0.95
    # scales: every option is away from its default, and each one changes the chains
    o = scales.opts
    assert (o.drscale, o.adascale, o.qcovadj, o.burnin_scale) == (3.0, 0.7, 1e-3, 4.0)
    for field, default in (("drscale", 5.0), ("adascale", 0.0), ("qcovadj", 1e-5), ("burnin_scale", 10.0)):
        other = scales.run_restatement(c_oracle, opts=dataclasses.replace(o, **{field: default}))
        assert any(not np.array_equal(other["R"][k], scales.want["R"][k]) for k in _chains(scales)), field


@pytest.mark.parametrize("group", GROUPS)
def test_burnin_only_and_no_adapt_keep_the_closed_forms(c_oracle, group):
    case = D.build(group, "burnin_only", c_oracle)
    assert case.opts.burnintime > case.opts.n_steps and D.burnin_windows(case) == case.opts.n_steps // case.opts.adaptint
    scaled = 0
    for k in _chains(case):
        R, R0 = _R(case, k), _R0(case, k)
        assert np.all(R[~np.eye(len(R), dtype=bool)] == 0.0)
        f = np.diag(R) / np.diag(R0)
        np.testing.assert_allclose(f, f[0], rtol=1e-14)  # one factor for the whole diagonal
        scaled += f[0] != 1.0
    assert scaled > 0  # and some chain was scaled
    case = D.build(group, "no_adapt", c_oracle)
    assert case.opts.adaptint == 0
    for k in _chains(case):
        np.testing.assert_array_equal(_R(case, k), _R0(case, k))


@pytest.mark.parametrize("group", GROUPS)
def test_ragged_schedule_is_off_every_grid(c_oracle, group):
    case = D.build(group, "ragged", c_oracle)
    o = case.opts
    assert o.burnintime % o.adaptint and o.n_steps % o.adaptint and (o.stats_from - 1) % o.thin
    assert (o.stats_from - 1) % o.adaptint and o.thin > 1 and (o.n_steps - 1) % o.thin
    first_cov = -(-o.burnintime // o.adaptint) * o.adaptint
    assert first_cov // o.adaptint >= 3 and first_cov + o.adaptint <= o.n_steps  # spans 3 windows; a recurrence follows
    for k in _chains(case):
        X = _rows(case, k)[o.stats_from - 1:]
        P = 7 + int(case.n[k])
        np.testing.assert_allclose(case.want["mean"][k, :P], X.mean(0), rtol=0, atol=1e-12 * np.abs(X).max())
        np.testing.assert_allclose(case.want["std"][k, :P], X.std(0), rtol=0, atol=1e-10 * np.abs(X).max())
        assert np.any(np.triu(_R(case, k), 1) != 0.0)  # adapted


@pytest.mark.parametrize("group", GROUPS)
def test_burnin_zero_adapts_from_the_first_window(c_oracle, group):
    """R'R = sc^2 (cov(rows 1..n_steps) + qcovadj I): row 1 included, no window skipped."""
    case = D.build(group, "burnin_zero", c_oracle)
    o = case.opts
    assert o.burnintime == 0 and o.n_steps % o.adaptint == 0
    for k in _chains(case):
        P = 7 + int(case.n[k])
        want = (2.4 ** 2 / P) * (np.cov(_rows(case, k).T, ddof=1) + o.qcovadj * np.eye(P))
        R = _R(case, k)
        np.testing.assert_allclose(R.T @ R, want, rtol=1e-9, atol=1e-9 * np.abs(want).max())
    one = case.run_restatement(c_oracle, opts=dataclasses.replace(o, n_steps=o.adaptint))
    assert all(np.any(np.triu(one["R"][k], 1) != 0.0) for k in _chains(case))  # adapted at the first window


@pytest.mark.parametrize("group", GROUPS)
def test_core_priors_change_the_decisions(c_oracle, group):
    case = D.build(group, "priors", c_oracle)
    sig = case.prior_sig.copy()
    assert np.all(np.isfinite(sig[:, :7])) and np.all(case.prior_mu[:, :7] != 0.0)
    assert np.allclose(np.abs(case.prior_mu[:, :7] - case.theta0[:, :7]), sig[:, :7])
    for k in _chains(case):
        P = 7 + int(case.n[k])
        assert np.all(case.prior_mu[k, 7:P] == D.PRIOR_RATE[0]) and np.all(sig[k, 7:P] == D.PRIOR_RATE[1])
    sig[:, :7] = np.inf
    flat = case.run_restatement(c_oracle, prior_sig=sig)
    differ = [not np.array_equal(D.moved_mask(_rows(case, k)), D.moved_mask(flat["chain"][:, k, :7 + int(case.n[k])]))
              for k in _chains(case)]
    assert any(differ), differ  # the likelihood alone decides in some chains
    base = D.build(group, "baseline", c_oracle)  # and the rate prior differs from the default N(0, 50)
    assert not np.array_equal(flat["chain"], base.want["chain"])


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("name", ["hierarchical", "tight_box"])
def test_bounds_reach_every_delayed_rejection_path(c_oracle, group, name):
    """Stage 1 out of bounds then stage 2 in bounds; stage 1 in bounds and rejected then stage 2 in bounds;
    stage 2 out of bounds; a stage 2 accepted after an out-of-bounds stage 1 (ss1 = Inf, pr1 = 0)."""
    case = D.build(group, name, c_oracle)
    counts = case.want["dr_counts"]
    assert np.all(counts.sum(axis=0) >= 10), counts
    if name == "tight_box":
        assert np.all(counts >= 5), counts  # in every chain
    steps = case.opts.n_steps - 1
    for k in _chains(case):
        assert counts[k, :3].sum() <= steps and D.moved_mask(_rows(case, k)).sum() >= counts[k, 3]
        # every in-bounds proposal is one evaluation: at least the in-bounds stage 2's, at most two a step less those known out of bounds
        assert 1 + counts[k, 0] + counts[k, 1] <= case.want["n_evals"][k] <= 1 + 2 * steps - counts[k, 0] - counts[k, 2]
    if name == "hierarchical":
        for k in _chains(case):
            v0 = D.hierarchical_v0(len(case.n))[k]
            assert 0.0 < v0 < 10.0 and case.lower[k, 0] == v0 - 1e-5 and case.upper[k, 0] == v0 + 1e-5
            assert counts[k, 0] + counts[k, 2] > 0.8 * counts[k, :3].sum()  # most stage-2 steps meet a bound
    else:
        base = D.build(group, "baseline", c_oracle)
        narrowed = (case.lower != base.lower) | (case.upper != base.upper)
        assert np.all(narrowed.sum(axis=1) == len(D.TIGHT_BOX_COORDS))


@pytest.mark.parametrize("group", GROUPS)
def test_frozen_chain_never_moves_and_keeps_its_factor(c_oracle, group):
    case = D.build(group, "frozen", c_oracle)
    o = case.opts
    assert o.qcovadj == 0.0
    k_scaled = D.burnin_windows(case)
    assert k_scaled == 2
    for k in _chains(case):
        P = 7 + int(case.n[k])
        th0 = case.theta0[k, :P]
        np.testing.assert_array_equal(th0 * 1024.0, np.round(th0 * 1024.0))
        assert case.lower[k, D.FROZEN_COORD] == case.upper[k, D.FROZEN_COORD] == th0[D.FROZEN_COORD]
        assert (case.lower[k, :P] == case.upper[k, :P]).sum() == 1
        np.testing.assert_array_equal(_rows(case, k), np.broadcast_to(th0, (o.n_steps, P)))
        # exact column sums and means: the window's covariance is exactly zero in any summation order
        assert np.all(np.abs(th0) * o.n_steps < 2.0 ** 42)
        want = _R0(case, k)
        for _ in range(k_scaled):
            want = want / o.burnin_scale
        np.testing.assert_array_equal(_R(case, k), want)
        assert np.all(D.window_rejection_rates(case, k) > 0.95)
    np.testing.assert_array_equal(case.want["n_evals"], 1)
    np.testing.assert_array_equal(case.want["accept_rate"], 0.0)
    np.testing.assert_array_equal(case.want["dr_counts"], np.array([0, 0, o.n_steps - 1, 0]) + 0 * case.want["dr_counts"])
