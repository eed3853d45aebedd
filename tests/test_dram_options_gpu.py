"""The GPU sampler against the CPU restatement across the option space (MI355X).

test_dram_gpu.py's restatement tests run one point of the option space (ntry = 2, updatesigma, drscale = 5,
adascale = 0, qcovadj = 1e-5, burnin_scale = 10, thin = 1, adaptint dividing burnintime, sigma2_0 = 1,
plan_fit's bounds and priors). Here every engine (FUSED k_chain, WALK k_walk, BATCHED k_accept1 / k_accept2)
and every adaptation kernel follows the restatement (oracle/tci_dram_oracle.c, run_chain) through the other
branches, with _follows_the_restatement's assertions and tolerances: the same accept / reject decision at
every step, rows, s2chain, mean, sigma_mean and R within 1e-9, std within 1e-7, n_evals equal -- and
accept_rate equal, final_theta the last row, sigma_std within 1e-9.

Groups (tests/dram_option_cases.py; synthetic cells, two per length):
  small  N = 9 and 40   P = 16, 47 under one ld, RPL = 1, k_adapt_mfma<8, 9, 6, 4>
  mid    N = 150        P = 157, RPL = 4, k_adapt_mfma<8, 13, 12>
  gt     N = 210        P = 217, RPL = 4, k_adapt_gt

Cases and the branch each one reaches (tests/test_oracle_dram_options.py asserts on the restatement alone
that it does):
  am            ntry = 1: no stage 2, step for step
  fixed_sigma   updatesigma = False, another sigma2_0 per chain: s2chain is sigma2_0 bit for bit
  scales        drscale = 3 (R / 3 against R * (1 / 3)), adascale = 0.7, qcovadj = 1e-3, burnin_scale = 4;
                a burn-in window above 0.95 rejections: R / burnin_scale
  burnin_up     qcov_diag * 1e-8: burn-in windows below 0.05 rejections: R * burnin_scale
  burnin_only   burnintime > n_steps: scaling only, the off-diagonal of R exactly 0
  no_adapt      adaptint = 0: R = diag(sqrt(qcov_diag)) bit for bit
  ragged        adaptint = 64, burnintime = 150, n_steps = 333, stats_from = 77, thin = 5: the first covariance
                update spans three windows, a tail window never adapts, kept rows and statistics off the grid
  burnin_zero   burnintime = 0: the first window, row 1 included, goes into the covariance
  priors        finite priors on the core parameters, prior_mu one prior_sig from x0, N(2, 5) on the rates
                (prior_ss, wave_prior, wave_prior_reg, the evaluation's fused prior_part)
  hierarchical  plan_fit(v0=...): v0 +- 1e-5, stage 1 out of bounds at almost every step (ss1 = Inf, pr1 = 0)
  tight_box     x0 +- sqrt(qcov_diag) on v, tau and one rate: all four combinations of stage 1 / stage 2
                in or out of bounds
  frozen        lower == upper == theta0 on tau, theta0 in multiples of 2^-10, qcovadj = 0: no proposal in
                bounds, the covariance exactly zero, the Cholesky fails at its first pivot ("cmat singular,
                not adapting"): R is the initial factor over burnin_scale^2, n_evals = 1, accept_rate = 0

Largest errors on the MI355X over the 108 runs (the three engines of a run agree): rows 2.5e-11 relative to
max(|row|, 1) and R 5.1e-12 of max|R|, both in am / gt; by case, rows / R: am 2.5e-11 / 5.1e-12, fixed_sigma
2.8e-12 / 2.6e-12, scales 4.0e-12 / 7.3e-13, burnin_up 1.5e-14 / 8.4e-13, burnin_only 6.7e-15 / 1.7e-16,
no_adapt 6.7e-15 / 0, ragged 6.2e-12 / 1.9e-12, burnin_zero 4.6e-12 / 2.8e-12, priors 6.6e-12 / 2.5e-12,
hierarchical 1.4e-12 / 2.5e-12, tight_box 3.0e-12 / 1.7e-12, frozen 0 / 1.7e-16 (R * (1 / 10) against R / 10).
"""
import dataclasses

import numpy as np
import pytest

import dram_option_cases as D
from test_dram_gpu import _adapt_kernel, _assert_follows_the_restatement

pytestmark = pytest.mark.gpu

ENGINES = ("fused", "walk", "batched")


def _gpu_run(case, engine):
    """One GPU run of the case (-> result, rows per lane of the context)."""
    from transcriptioncycleinference_amd import Likelihood
    from transcriptioncycleinference_amd.mcmc import dram_run

    o = dataclasses.replace(case.opts, engine=engine)
    with Likelihood(case.cells, case.construct, device=0) as L:
        rpl = L.info["rows_per_lane"]
        g = dram_run(L, case.cell_id, case.theta0, case.lower, case.upper, case.prior_mu, case.prior_sig,
                     case.qcov_diag, case.sigma2_0, o, chain_keys=case.keys, want_qcov=True)
    return g, rpl


def _kept(case):
    """The restatement's outputs with the rows the GPU keeps (chain row 1 + k thin)."""
    thin = int(case.opts.thin)
    c = dict(case.want)
    c["chain"], c["s2chain"] = case.want["chain"][::thin], case.want["s2chain"][::thin]
    return c


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("group", sorted(D.GROUPS))
@pytest.mark.parametrize("name", D.CASES)
def test_gpu_chains_follow_the_cpu_restatement_across_the_options(c_oracle, name, group, engine):
    case = D.build(group, name, c_oracle)
    o, n, c = case.opts, case.n, _kept(case)
    g, rpl = _gpu_run(case, engine)
    assert g.chain.shape == c["chain"].shape
    for k in range(len(n)):  # the first step at which the decisions differ, before anything fails
        P = 7 + int(n[k])
        mg, mc = D.moved_mask(g.chain[:, k, :P]), D.moved_mask(c["chain"][:, k, :P])
        if not np.array_equal(mg, mc):
            i = int(np.flatnonzero(mg != mc)[0])
            print(f"options {name} {group} {engine}: chain {k} first differs at kept row {i + 2} (chain row "
                  f"{(i + 1) * o.thin + 1}): GPU moved {bool(mg[i])}, restatement moved {bool(mc[i])}")
    assert _adapt_kernel(D.GROUP_EXPECT[group][0]) == D.GROUP_EXPECT[group][2]
    _assert_follows_the_restatement(f"{name} {group}", engine, n, g, rpl, c, D.GROUP_EXPECT[group])
    np.testing.assert_array_equal(g.accept_rate, c["accept_rate"])
    np.testing.assert_allclose(g.sigma_std, c["sigma_std"], rtol=1e-9, atol=1e-9)
    for k in range(len(n)):
        P = 7 + int(n[k])
        np.testing.assert_allclose(g.final_theta[k, :P], case.want["chain"][-1, k, :P], rtol=1e-9, atol=1e-9)
        if (o.n_steps - 1) % o.thin == 0:
            np.testing.assert_array_equal(g.final_theta[k, :P], g.chain[-1, k, :P])
        R, R0 = g.qcov_R[k, :P, :P], np.diag(np.sqrt(case.qcov_diag[k, :P]))
        if name == "fixed_sigma":
            np.testing.assert_array_equal(g.s2chain[:, k], np.asarray(case.sigma2_0)[k])
        if name in ("burnin_only", "frozen"):
            assert np.all(R[~np.eye(P, dtype=bool)] == 0.0)
        if name == "no_adapt":
            np.testing.assert_array_equal(R, R0)
        if name == "frozen":
            assert g.n_evals[k] == 1 and g.accept_rate[k] == 0.0
            np.testing.assert_array_equal(g.chain[:, k, :P], np.broadcast_to(case.theta0[k, :P], (o.n_steps, P)))
            np.testing.assert_allclose(R, R0 / o.burnin_scale ** D.burnin_windows(case), rtol=1e-9, atol=0)
    if name == "ragged":
        assert g.chain.shape[0] == (o.n_steps + o.thin - 1) // o.thin
