"""Fit driver: the reference's per-cell MCMC setup + the GPU-resident batched DRAM + its outputs.

Mirrors ``src/TranscriptionCycleMCMC.m``:

* per-cell setup (``:161-270``): truncation, ``data``, x0 (``:193-210``), the proposal
  covariance J0 (``:214-231``), bounds (``:233-255``), Gaussian priors on dR (``:254``),
  ``model.sigma2 = 1`` (``:212,259``);
* ``mcmcrun`` (``:273``) -> :func:`dram_run` (``tci_dram_run``: all chains at once on the GPU);
* summaries (``:275-303``), the forward model at the means (``:305-309``), the
  ``MCMCchain`` / ``MCMCresults`` / ``MCMCplot`` structs (``:149-157,315-356``), the pruning of
  skipped cells (``:359-369``) and the two result files (``:371-378``).

The reference runs cells in a parfor with independent MATLAB RNG streams (``rand``/``normrnd``).
Here x0 comes from ``numpy.random.default_rng([seed, cell])`` and the chains from Philox streams, so a
fit reproduces the reference's *distribution*, not its exact draws.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import datetime
import math
import os
from dataclasses import dataclass, field
from typing import Dict, List, Mapping, Optional, Sequence

import numpy as np

from . import _lib
from .data import Cells, draw_x0
from .likelihood import (FITCHECK_POINTWISE, ChainCov, ChainDens, ChainEss, ChainLp, ChainQuant, ChainRank, ChainRhat, ChainStats,
                         Demc, DemcZs, FitCheck, ModeSearch, rhat_groups)

RESULT_FIELDS = ("mean_v", "sigma_v", "mean_ton", "sigma_ton", "mean_A", "sigma_A", "mean_tau", "sigma_tau",
                 "mean_MS2_basal", "sigma_MS2_basal", "mean_PP7_basal", "sigma_PP7_basal", "mean_R", "sigma_R",
                 "mean_dR", "sigma_dR", "mean_sigma", "sigma_sigma", "cell_index", "ApprovedFits")  # :151-155
CHAIN_FIELDS = ("v_chain", "ton_chain", "A_chain", "tau_chain", "MS2_basal_chain", "PP7_basal_chain", "R_chain",
                "dR_chain", "s2chain")  # :149-150
PLOT_FIELDS = ("t_plot", "MS2_plot", "PP7_plot", "simMS2", "simPP7")  # :156-157
PRED_FIELDS = ("predMS2", "predPP7", "pred_probs")  # added to MCMCplot by :func:`predict`
_SCALARS = ("v", "ton", "A", "tau", "MS2_basal", "PP7_basal", "R")
# MCMCdiag (fit(..., diagnostics=True)): chain diagnostics per fitted cell, mcmcstat's chainstats columns
DIAG_FIELDS = (tuple(f"{s}_{n}" for s in ("mcerr", "tau", "geweke_p") for n in _SCALARS + ("dR", "s2"))
               + ("n_rows", "ess_min", "cell_index"))
# MCMCcov (fit(..., covariance=True)): posterior mean, covariance and correlation per fitted cell, P = 7 + N wide
COV_FIELDS = ("mean", "cov", "corr", "n_rows", "cell_index")
# MCMCquant (fit(..., quantiles=probs)): posterior quantiles per fitted cell, [nq] per parameter at `probs`
QUANT_FIELDS = tuple("q_" + s for s in _SCALARS) + ("q_dR", "q_s2", "probs", "n_rows", "cell_index")
# MCMCdens (fit(..., density=True)): marginal density and histogram per fitted cell, P + 1 = 7 + N + 1 columns wide
# (theta order, s2 last): grid, dens [G, P + 1], counts [B, P + 1], range [2, P + 1], bw [P + 1]
DENS_FIELDS = ("grid", "dens", "counts", "range", "bw", "n_rows", "cell_index")
# MCMCrhat (fit(..., replicates=M) or fit(..., rhat=True)): convergence across the M replicate chains of a fitted cell,
# P + 1 = 7 + N + 1 columns wide (theta order, s2 last): rhat, rhat_split, pooled_mean, pooled_std [P + 1];
# mean_rep [M, P] and accept_rep [M]: every replicate's posterior means and acceptance rate; rhat_max: the largest
# classic or split factor of the cell
RHAT_FIELDS = ("rhat", "rhat_split", "pooled_mean", "pooled_std", "mean_rep", "accept_rep", "rhat_max", "n_rows",
               "n_chains", "cell_index")
# MCMCess (fit(..., replicates=M, ess=True)): the multi-chain effective sample size of a fitted cell, P + 1 = 7 + N + 1
# columns wide (theta order, s2 last): ess, ess_split, tau, tau_split, mcse [P + 1] doubles, window, window_split
# [P + 1] int32; ess_min: the smallest classic or split ess of the cell; max_lag: the cap the fit passed (0 = none)
ESS_FIELDS = ("ess", "ess_split", "tau", "tau_split", "mcse", "window", "window_split", "ess_min", "max_lag", "n_rows",
              "n_chains", "cell_index")
# MCMCrank (fit(..., replicates=M, rank=True)): the rank diagnostics of a fitted cell (include/tci.h, tci_chainrank),
# P + 1 = 7 + N + 1 columns wide (theta order, s2 last): q [nq, P + 1] at probs [nq], q_tail [2, P + 1] at tail [2],
# the R-hat, ESS and tau vectors [P + 1] doubles, the windows [P + 1] int32; rhat_rank_max, ess_bulk_min, ess_tail_min:
# the cell's worst values, NaN left out; max_lag: the cap the fit passed (0 = none)
RANK_VECTORS = ("rhat_bulk", "rhat_folded", "rhat_rank", "ess_bulk", "tau_bulk", "ess_tail_lo", "ess_tail_hi", "ess_tail",
                "window_bulk", "window_tail_lo", "window_tail_hi")
RANK_FIELDS = ("q", "q_tail", "probs", "tail") + RANK_VECTORS + ("rhat_rank_max", "ess_bulk_min", "ess_tail_min",
                                                                 "max_lag", "n_rows", "n_chains", "cell_index")
# MCMCcheck (fitcheck(lk, fit_result)): posterior predictive fit checks per fitted cell (include/tci.h): the pointwise
# vectors [2, N] (row 0 = MS2, row 1 = PP7; NaN where a point is not scored), the per-cell scalars, coverage [n_levels]
# at levels, dw [2] per dye
CHECK_FIELDS = FITCHECK_POINTWISE + ("n_obs", "lppd", "p_waic", "elpd_waic", "waic", "chi2", "coverage", "dw", "levels",
                                     "n_samples", "cell_index")
# MCMClp (fit(..., logpost=True)): the log-posterior trace of a fitted cell (include/tci.h, tci_chainlp). With one chain
# per cell the scalars are floats, best_row an int, best_<name> the best sample split into the reference's parameter
# names (best_dR [N]) and ss / lp the traces [n_rows] (ss: mcmcstat's sschain). With replicates = M every one of those
# gains a leading axis of M (the traces become [M, n_rows]) and the cell also carries LP_GROUP_FIELDS: R-hat (classic
# and split), the multi-chain ESS and the MCSE of lp across the replicates, ss_gap = max_r ss_mean - min_r ss_mean and
# best_replicate, the replicate of the largest lp_best (-1 when every one is NaN)
LP_SCALARS = _lib.CHAINLP_SCALARS
LP_FIELDS = (LP_SCALARS + ("best_row",) + tuple("best_" + s for s in _SCALARS) + ("best_dR", "ss", "lp", "n_rows",
                                                                                  "n_chains", "cell_index"))
LP_GROUP_FIELDS = ("lp_rhat", "lp_rhat_split", "lp_ess", "lp_mcse", "ss_gap", "best_replicate")
# MCMCstack (fit(..., stack=nsample)): PSIS-LOO of every replicate of a fitted cell and the stacking weights across them
# (include/tci.h, tci_loocheck): weights [M]; per replicate [M] elpd_loo, p_loo, khat_max, n_khat_bad; replicate 0's
# pointwise elpd_loo_i and khat_i [2, N]; elpd_stack; stacked_mean [7 + N] = sum_r weights_r * (replicate r's posterior
# mean).
STACK_FIELDS = ("weights", "elpd_loo", "p_loo", "khat_max", "n_khat_bad", "elpd_loo_i", "khat_i", "elpd_stack",
                "stacked_mean", "n_samples", "cell_index")
# MCMCtemper (fit(..., temper=R)): the ladder of a fitted cell: beta [R]; per replicate the swap acceptance of every
# pair of neighbouring rungs, swap_rate [M, R - 1] (NaN for a pair never tried) with swap_tried [M, R - 1], and every
# rung's DRAM acceptance rate, accept_rate [M, R]
TEMPER_FIELDS = ("beta", "swap_rate", "swap_tried", "accept_rate", "swap_every", "n_events", "n_chains", "cell_index")
# MCMCsearch (fit(..., presearch=dict(...))): the mode search that chose the chains' starts (include/tci.h,
# tci_modesearch): the best member's f, ss and theta [7 + N], f0_best the best f of the initial population, f_trace
# [n_gen + 1] the best f after every generation, n_evals the cell's SS evaluations
SEARCH_FIELDS = ("f_best", "ss_best", "theta_best", "f0_best", "f_trace", "n_gen", "n_pop", "n_evals", "cell_index")
PRESEARCH_KEYS = ("n_pop", "n_gen", "F", "CR")
# MCMCdemc (fit(..., demc=dict(...))): the DE-MC population sampler's per-cell record
DEMC_FIELDS = ("accept_rate", "n_oob", "rhat_max", "ess_min", "n_pop", "n_gen", "n_evals", "cell_index")
DEMC_KEYS = ("n_pop", "n_gen", "CR", "gamma0", "jump_every", "jitter", "updatesigma")
# MCMCdemczs (fit(..., demczs=dict(...))): the DE-MC(zs) sampler's per-cell record: MCMCdemc's fields plus the null
# snooker moves per chain, the share of snooker moves (NaN without the log), the starting and the final archive rows
# With census (tci_demczs_run_bounds): n_cross, oob_lo, oob_hi [7 + N] summed over the cell's chains, and oob_share
# [7 + N], the share of the bounds-rejected proposals in which coordinate j had left. With bounds='reflect':
# reflect_rate, the share of all proposals that were evaluated after at least one reflection. None when the feature is off.
DEMCZS_FIELDS = DEMC_FIELDS + ("n_null", "snooker_rate", "m0", "n_archive", "n_cross", "oob_lo", "oob_hi", "oob_share",
                               "reflect_rate")
DEMCZS_KEYS = DEMC_KEYS + ("m0", "append_every", "p_snooker", "bounds", "census")
ZS_FIT_LOG_ROWS = 1024   # the generations a demczs fit logs: snooker_rate is the share of snooker moves among them
# RNG stream key of replicate r of dataset-wide cell g: g + r * REPLICATE_KEY_STRIDE. The sampler's Philox counter
# carries the low 32 bits of a chain's key and nothing else of it (include/tci.h, chain_keys), so the replicate has to
# sit there: cells below 2^24, at most 2^8 replicates, and every key below 2^32.
REPLICATE_KEY_STRIDE = 1 << 24
MAX_REPLICATES = 1 << 8
THETA_INDEX = {"v": 0, "tau": 1, "ton": 2, "MS2_basal": 3, "PP7_basal": 4, "A": 5, "R": 6}


@dataclass
class DramOptions:
    """``options`` of ``TranscriptionCycleMCMC.m:263-270`` plus mcmcstat's DRAM defaults."""

    n_steps: int = 20000          # options.nsimu = n_steps (:264; default :40)
    burnintime: int = 10000       # options.burnintime = n_burn (:267; default :39)
    adaptint: int = 100           # :268
    ntry: int = 2                 # 'dram' (:269)
    updatesigma: bool = True      # :265
    drscale: float = 5.0
    adascale: float = 0.0         # 0: 2.4/sqrt(npar)
    qcovadj: float = 1e-5
    burnin_scale: float = 10.0
    stats_from: int = 10000       # chain(n_burn:end, :) (:276)
    thin: int = 0
    seed: int = 20201028
    engine: str = "auto"          # "auto" | "fused" | "batched" | "walk" (include/tci.h TCI_DRAM_*): identical chains
    max_chunk: int = 0            # FUSED/WALK rows per draws pass + walk (0 = automatic); identical chains
    adapt_pmax: int = 0           # a shard of a larger fit: that fit's largest P (the adaptation kernel's pick)
    kernel_times: bool = False    # FUSED/WALK: HIP-event device time per kernel class (DramResult.kernel_ms)

    ENGINES = {"auto": 0, "fused": 1, "batched": 2, "walk": 3}

    def to_c(self, chain_keys: Optional[np.ndarray] = None) -> "_lib.tci_dram_options":
        """``chain_keys`` (int64 [n_chains], kept alive by the caller): chain c's RNG stream key."""
        if self.engine not in self.ENGINES:
            raise ValueError(f"engine must be one of {sorted(self.ENGINES)}, got {self.engine!r}")
        return _lib.tci_dram_options(int(self.n_steps), int(self.burnintime), int(self.adaptint), int(self.ntry),
                                     int(bool(self.updatesigma)), float(self.drscale), float(self.adascale),
                                     float(self.qcovadj), float(self.burnin_scale), int(self.stats_from),
                                     int(self.thin), int(self.seed) & 0xFFFFFFFFFFFFFFFF,
                                     self.ENGINES[self.engine], int(self.max_chunk), _lib.ptr(chain_keys, _lib._i64p),
                                     int(self.adapt_pmax), int(bool(self.kernel_times)))


@dataclass
class DramResult:
    mean: np.ndarray
    std: np.ndarray
    final_theta: np.ndarray
    sigma_mean: np.ndarray
    sigma_std: np.ndarray
    accept_rate: np.ndarray
    n_evals: np.ndarray
    chain: Optional[np.ndarray]
    s2chain: Optional[np.ndarray]
    elapsed_ms: float
    qcov_R: Optional[np.ndarray] = None   # final proposal factor (upper, R'R = mcmcstat results.qcov)
    kernel_ms: Optional[np.ndarray] = None        # DramOptions.kernel_times: ms per class (draws, walk, adapt,
    #                                               the split draws' first-chunk launch; include/tci.h)
    kernel_launches: Optional[np.ndarray] = None  # and launches per class
    temper: Optional["TemperResult"] = None       # dram_run(beta=, ladder=): the ladders and their swap records
    lp: Optional[ChainLp] = None                  # dram_run(logpost=True): log-posterior trace, best sample, DIC
    ess: Optional[ChainEss] = None                # dram_run(group=ids, ess=True): effective sample size of every group
    rank: Optional[ChainRank] = None              # dram_run(group=ids, rank=True): rank diagnostics of every group
    rhat: Optional[ChainRhat] = None              # dram_run(group=ids): R-hat / pooled moments of every group of chains
    dens: Optional[ChainDens] = None              # dram_run(dens=True): densities / histograms of the kept rows
    quant: Optional[ChainQuant] = None            # dram_run(quant=probs): quantiles of the kept rows
    stats: Optional[ChainStats] = None            # dram_run(stats=True): diagnostics of the kept rows
    cov: Optional[ChainCov] = None                # dram_run(cov=True): mean / cov / corr of the same rows


@dataclass
class TemperResult:
    """The ladders of a tempered run (``tci_dram_run_tempered``) and what their swaps did. Event ``e`` follows chain
    row ``event_rows[e]``; a pair's records sit at its lower rung (the chain of the larger beta)."""

    beta: np.ndarray            # [n_chains]
    ladder: np.ndarray          # [n_chains] int32, -1 = in no ladder
    swap_every: int
    swap_tried: np.ndarray      # [n_chains] int32
    swap_accepted: np.ndarray   # [n_chains] int32
    swap_logr: np.ndarray       # [n_events, n_chains], NaN where no pair was tried
    swap_acc: np.ndarray        # [n_events, n_chains] uint8
    event_rows: np.ndarray      # [n_events] int64: the 1-based chain row each event follows
    n_events: int = 0


def temper_ladder(P: int, rungs: int, ratio: Optional[float] = None) -> np.ndarray:
    """Inverse temperatures ``beta_r = ratio**r`` of a ladder of ``rungs`` rungs, cold first. The default ratio
    ``1 / (1 + sqrt(2 / P))`` is the geometric spacing that holds the swap acceptance constant along the ladder of a
    ``P``-dimensional Gaussian target (Kofke 2002; Predescu et al. 2004): the energy at beta has standard deviation
    ``sqrt(P / 2) / beta``, so neighbouring energy distributions overlap alike when ``(beta_r - beta_{r+1}) / beta_{r+1}``
    is ``sqrt(2 / P)``. It is derived, not tuned."""
    P, R = int(P), int(rungs)
    if P < 1 or R < 1:
        raise ValueError("temper_ladder needs P >= 1 and rungs >= 1")
    q = 1.0 / (1.0 + math.sqrt(2.0 / P)) if ratio is None else float(ratio)
    if not (0.0 < q < 1.0):
        raise ValueError("ratio must be in (0, 1)")
    return q ** np.arange(R, dtype=np.float64)


def swap_event_rows(n_steps: int, adaptint: int, swap_every: int) -> np.ndarray:
    """The 1-based chain rows the swap events of a run follow: the ends ``w * win`` of the windows (``win = adaptint``,
    or 100 without adaptation) with ``w % swap_every == 0`` that lie before the run's last row."""
    win = int(adaptint) if int(adaptint) > 0 else 100
    se = int(swap_every)
    n = (int(n_steps) - 1) // win // se if se > 0 else 0
    return (1 + np.arange(n, dtype=np.int64)) * se * win


def dram_run(lk, cell_id, theta0, lower, upper, prior_mu, prior_sig, qcov_diag, sigma2_0,
             opts: DramOptions, want_qcov: bool = False, chain_keys=None, stats: bool = False,
             max_lag: int = 0, want_chain: bool = True, cov: bool = False,
             cov_scratch_bytes: int = 0, quant=None, dens=None, group=None, ess: bool = False,
             logpost: bool = False, beta=None, ladder=None, swap_every: int = 1, rank=False) -> DramResult:
    """Run one chain per row on the device (``tci_dram_run``). Arrays are (n_chains, ld).
    ``want_qcov``: also return the final proposal factor R (n_chains, ld, ld). ``chain_keys``:
    RNG stream key per chain (default: the row index). ``stats``: also the chain diagnostics
    (``tci_dram_run_stats``) of the kept rows at or past ``opts.stats_from``, reduced from the device
    chain (``DramResult.stats``; needs ``opts.thin >= 1``; ``max_lag`` as in ``Likelihood.chainstats``).
    ``want_chain=False``: the kept rows are not copied to the host (``chain`` and ``s2chain`` are None).
    ``cov``: also the mean, covariance and correlation (``tci_dram_run_cov``) of those same rows, at least 2
    of them, reduced from the device chain (``DramResult.cov``; ``cov_scratch_bytes`` as ``scratch_bytes`` of
    ``Likelihood.chaincov``); works with or without ``stats``. ``quant``: a sequence of 1 to 16 probabilities:
    also the exact quantiles of those same rows at them (``DramResult.quant``, as ``Likelihood.chainquant``
    gives), selected from the device chain; the run then goes through ``tci_dram_run_reduced``, which takes any
    of the reductions. ``dens``: ``True`` or a dict of ``n_grid`` / ``n_bins`` / ``bw_scale``: also the marginal
    density and histogram of every column of those same rows, at least 2 of them (``DramResult.dens``, as
    ``Likelihood.chaindens`` gives), through ``tci_dram_run_reduced`` too. ``group``: one id per chain (-1 = none):
    also the classic and split R-hat and the pooled mean and standard deviation of every group of chains over those
    same rows, at least 2 of them (``DramResult.rhat``, as ``Likelihood.chainrhat`` gives), reduced from the device
    chain through ``tci_dram_run_rhat``, with any of the other reductions. ``ess`` (needs ``group``): also the
    multi-chain effective sample size of every group over those rows (``DramResult.ess``, as ``Likelihood.chainess``
    gives, with ``max_lag`` as its cap on the lags), through ``tci_dram_run_ess``. ``logpost``: also the sum-of-squares
    trace (mcmcstat's ``sschain``), the prior, deviance and log-posterior of every one of those same rows and per chain
    the best sample and DIC (``DramResult.lp``, as ``Likelihood.chainlp`` gives with the run's priors), from the device
    chain through ``tci_dram_run_lp``, with any of the other reductions. With ``logpost`` the priors are checked before
    the run as ``Likelihood.chainlp`` checks them: a ``prior_mu`` entry (of a chain's ``7 + N``) that is not finite, or a
    ``prior_sig`` entry that is NaN or <= 0, is a ``TciError`` (``TCI_EINVAL``) although the sampler alone would run.

    ``beta`` / ``ladder``: parallel tempering (``tci_dram_run_tempered``, include/tci.h). ``beta``: the inverse
    temperature of every chain (default 1); ``ladder``: one ladder id per chain (-1 or absent = in no ladder): the chains
    of a ladder, in ascending row order, are its rungs, cold first, and exchange states after every ``swap_every``-th
    window of ``adaptint`` rows (0 = never). ``sigma2_0`` is physical; every s2 output of a rung with ``beta < 1`` is
    ``sigma2 / beta``. The swap records come back as ``DramResult.temper``. Works with ``stats``, ``cov``, ``quant``,
    ``dens`` and ``group``; ``ess`` and ``logpost`` have no tempered entry point (ValueError).

    ``rank`` (needs ``group``): ``True`` or a dict of ``probs`` / ``tail``: also the rank-normalised split R-hat, bulk
    and tail ESS and pooled quantiles of every group over those rows (``DramResult.rank``, as ``Likelihood.chainrank``
    gives, ``max_lag`` as its cap on the lags), through ``tci_dram_run_rank``; not with ``logpost`` or a tempered run."""
    tempered = beta is not None or ladder is not None
    want_rank = rank is not None and rank is not False
    if want_rank and group is None:
        raise ValueError("rank needs group: the rank diagnostics are statistics of groups of chains")
    if want_rank and (tempered or logpost):
        raise ValueError("rank has no entry point with logpost or a tempered run")
    if tempered and (ess or logpost):
        raise ValueError("a tempered run (beta= / ladder=) takes stats, cov, quant, dens and group, not ess or logpost")
    if tempered and (isinstance(swap_every, bool) or int(swap_every) != swap_every or int(swap_every) < 0):
        raise ValueError("swap_every must be an integer >= 0")
    if ess and group is None:
        raise ValueError("ess=True needs group: the effective sample size is a statistic of groups of chains")
    f = lambda a: np.ascontiguousarray(a, np.float64)  # noqa: E731
    theta0, lower, upper, prior_mu, prior_sig, qcov_diag = map(f, (theta0, lower, upper, prior_mu, prior_sig,
                                                                    qcov_diag))
    n, ld = theta0.shape
    cid = np.ascontiguousarray(cell_id, np.int32)
    s20 = f(np.broadcast_to(np.asarray(sigma2_0, np.float64), (n,)))
    mean, std, fin = np.empty((n, ld)), np.empty((n, ld)), np.empty((n, ld))
    smean, sstd, acc = np.empty(n), np.empty(n), np.empty(n)
    nev = np.empty(n, np.int64)
    n_keep = (opts.n_steps + opts.thin - 1) // opts.thin if opts.thin > 0 else 0
    chain = np.empty((n_keep, n, ld)) if n_keep and want_chain else None
    s2c = np.empty((n_keep, n)) if n_keep and want_chain else None
    qR = np.empty((n, ld, ld)) if want_qcov else None
    out = _lib.tci_dram_outputs(_lib.ptr(mean, _lib._dp), _lib.ptr(std, _lib._dp), _lib.ptr(fin, _lib._dp),
                                _lib.ptr(smean, _lib._dp), _lib.ptr(sstd, _lib._dp), _lib.ptr(acc, _lib._dp),
                                _lib.ptr(nev, _lib._i64p), _lib.ptr(chain, _lib._dp), _lib.ptr(s2c, _lib._dp),
                                _lib.ptr(qR, _lib._dp), 0.0)   # kernel_ms / kernel_launches: zero-initialised
    keys = None if chain_keys is None else np.ascontiguousarray(chain_keys, np.int64)
    if keys is not None and keys.shape != (n,):
        raise ValueError("chain_keys must have one entry per chain")
    o = opts.to_c(keys)
    P = lambda a: _lib.ptr(a, _lib._dp)  # noqa: E731
    args = (lk._h, C.byref(o), n, _lib.ptr(cid, _lib._i32p), P(theta0), P(lower), P(upper), P(prior_mu), P(prior_sig),
            P(qcov_diag), P(s20), ld, C.byref(out))
    cs = cc = cq = cd = cr = ce = clp = ck = None
    sopt = sout = None
    if group is not None:
        grp, ng = rhat_groups(group, n)
        cr = ChainRhat.empty(ng, ld)
        if ess:
            ce = ChainEss.empty(ng, ld, max_lag)
        if want_rank:
            ck = ChainRank.empty(ng, ld, max_lag=max_lag, **({} if rank is True else dict(rank)))
    if quant is not None:
        cq = ChainQuant.empty(n, ld, quant)
    if dens is not None and dens is not False:
        cd = ChainDens.empty(n, ld, **({} if dens is True else dict(dens)))
    if stats:
        cs = ChainStats.empty(n, ld)
        sopt, sout = _lib.tci_chainstats_options(int(max_lag)), cs.to_c()
    if logpost:
        k0 = (max(int(opts.stats_from), 1) - 1 + opts.thin - 1) // opts.thin if opts.thin > 0 else 0
        clp = ChainLp.empty(max(n_keep - k0, 0), n, ld)
    tr = None
    if tempered:
        bt = np.ones(n) if beta is None else f(beta)
        ldr = np.full(n, -1, np.int32) if ladder is None else np.ascontiguousarray(ladder, np.int32)
        if bt.shape != (n,) or ldr.shape != (n,):
            raise ValueError("beta and ladder must have one entry per chain")
        rows = swap_event_rows(opts.n_steps, opts.adaptint, swap_every)
        ne = len(rows)
        tr = TemperResult(bt, ldr, int(swap_every), np.zeros(n, np.int32), np.zeros(n, np.int32),
                          np.full((ne, n), np.nan), np.zeros((ne, n), np.uint8), rows)
        topt = _lib.tci_temper_options(P(bt), _lib.ptr(ldr, _lib._i32p), int(ldr.max(initial=-1)) + 1, int(swap_every), 0)
        tout = _lib.tci_temper_outputs(_lib.ptr(tr.swap_tried, _lib._i32p), _lib.ptr(tr.swap_accepted, _lib._i32p),
                                       P(tr.swap_logr) if ne else None, _lib.ptr(tr.swap_acc, _lib._u8p) if ne else None,
                                       ne, 0)
    if tempered or cq is not None or cd is not None or cr is not None or clp is not None:
        red = _lib.tci_dram_reductions()
        if cq is not None:
            qopt, qout = cq.options(), cq.to_c()
            red.qopt, red.qout = C.pointer(qopt), C.pointer(qout)
        if cd is not None:
            dopt, dout = cd.options(), cd.to_c()
            red.dopt, red.dout = C.pointer(dopt), C.pointer(dout)
        if stats:
            red.sopt, red.sout = C.pointer(sopt), C.pointer(sout)
        if cov:
            cc = ChainCov.empty(n, ld)
            copt, cout = _lib.tci_chaincov_options(int(cov_scratch_bytes)), cc.to_c()
            red.copt, red.cout = C.pointer(copt), C.pointer(cout)
        if tempered:          # tci_dram_run_tempered: the reductions and, with group, the group reduction
            ropt = rout = None
            if cr is not None:
                ropt, rout = cr.options(), cr.to_c()
            lk._check(lk._lib.tci_dram_run_tempered(*args, C.byref(red),
                                                    _lib.ptr(grp, _lib._i32p) if cr is not None else None,
                                                    ng if cr is not None else 0, None if ropt is None else C.byref(ropt),
                                                    None if rout is None else C.byref(rout), C.byref(topt),
                                                    C.byref(tout)))
            tr.n_events = int(tout.n_events)
            if cr is not None:
                cr.n_rows, cr.kernel_ms = int(rout.n_rows), float(rout.kernel_ms)
        elif clp is not None:   # tci_dram_run_lp takes every other reduction with it
            lopt, lout = clp.options(), clp.to_c()
            ropt = rout = eopt = eout = None
            if cr is not None:
                ropt, rout = cr.options(), cr.to_c()
            if ce is not None:
                eopt, eout = ce.options(), ce.to_c()
            ref = lambda x: None if x is None else C.byref(x)  # noqa: E731
            lk._check(lk._lib.tci_dram_run_lp(*args, C.byref(red), _lib.ptr(grp, _lib._i32p) if cr is not None else None,
                                              ng if cr is not None else 0, ref(ropt), ref(rout), ref(eopt), ref(eout),
                                              C.byref(lopt), C.byref(lout)))
            clp.n_rows, clp.kernel_ms = int(lout.n_rows), float(lout.kernel_ms)
            if cr is not None:
                cr.n_rows, cr.kernel_ms = int(rout.n_rows), float(rout.kernel_ms)
            if ce is not None:
                ce.n_rows, ce.kernel_ms = int(eout.n_rows), float(eout.kernel_ms)
        elif cr is not None:
            ropt, rout = cr.options(), cr.to_c()
            if ck is not None:
                eopt, eout = (ce.options(), ce.to_c()) if ce is not None else (None, None)
                kopt, kout = ck.options(), ck.to_c()
                lk._check(lk._lib.tci_dram_run_rank(*args, C.byref(red), _lib.ptr(grp, _lib._i32p), ng, C.byref(ropt),
                                                    C.byref(rout), None if eopt is None else C.byref(eopt),
                                                    None if eout is None else C.byref(eout), C.byref(kopt),
                                                    C.byref(kout)))
                ck.taken(kout)
                if ce is not None:
                    ce.n_rows, ce.kernel_ms = int(eout.n_rows), float(eout.kernel_ms)
            elif ce is not None:
                eopt, eout = ce.options(), ce.to_c()
                lk._check(lk._lib.tci_dram_run_ess(*args, C.byref(red), _lib.ptr(grp, _lib._i32p), ng, C.byref(ropt),
                                                   C.byref(rout), C.byref(eopt), C.byref(eout)))
                ce.n_rows, ce.kernel_ms = int(eout.n_rows), float(eout.kernel_ms)
            else:
                lk._check(lk._lib.tci_dram_run_rhat(*args, C.byref(red), _lib.ptr(grp, _lib._i32p), ng, C.byref(ropt),
                                                    C.byref(rout)))
            cr.n_rows, cr.kernel_ms = int(rout.n_rows), float(rout.kernel_ms)
        else:
            lk._check(lk._lib.tci_dram_run_reduced(*args, C.byref(red)))
        if cq is not None:
            cq.n_rows, cq.kernel_ms = int(qout.n_rows), float(qout.kernel_ms)
        if cd is not None:
            cd.n_rows, cd.kernel_ms = int(dout.n_rows), float(dout.kernel_ms)
        if cov:
            cc.n_rows, cc.kernel_ms = int(cout.n_rows), float(cout.kernel_ms)
    elif cov:
        cc = ChainCov.empty(n, ld)
        copt, cout = _lib.tci_chaincov_options(int(cov_scratch_bytes)), cc.to_c()
        lk._check(lk._lib.tci_dram_run_cov(*args, C.byref(sopt) if stats else None, C.byref(sout) if stats else None,
                                           C.byref(copt), C.byref(cout)))
        cc.n_rows, cc.kernel_ms = int(cout.n_rows), float(cout.kernel_ms)
    elif stats:
        lk._check(lk._lib.tci_dram_run_stats(*args, C.byref(sopt), C.byref(sout)))
    else:
        lk._check(lk._lib.tci_dram_run(*args))
    if stats:
        cs.n_rows, cs.kernel_ms = int(sout.n_rows), float(sout.kernel_ms)
    return DramResult(mean, std, fin, smean, sstd, acc, nev, chain, s2c, float(out.elapsed_ms), qcov_R=qR,
                      kernel_ms=np.array(out.kernel_ms[:], np.float64),
                      kernel_launches=np.array(out.kernel_launches[:], np.int64), lp=clp, ess=ce, rhat=cr, dens=cd, quant=cq, stats=cs,
                      cov=cc, temper=tr, rank=ck)


# ---------------------------------------------------------------------------
# TranscriptionCycleMCMC.m per-cell setup
# ---------------------------------------------------------------------------


def cell_setup(t: np.ndarray, rng: np.random.Generator, ratePriorWidth: float = 50.0,
               v0: Optional[float] = None):
    """x0, lower, upper, prior mu/sig and J0 diagonal for one cell (TranscriptionCycleMCMC.m:193-255).
    ``v0`` given = the hierarchical fit (loadPrevious): v fixed to v0 +- 1e-5 with step 1e-7."""
    n = len(t)
    x0 = draw_x0(rng, n, v0)                                                 # :200-210
    load_prev = v0 is not None
    v_step = 1e-7 if load_prev else 0.05                                      # :217-221
    ton_step = t[-1] - t[-2]                                                  # :222
    J0 = np.concatenate([[v_step, 0.1, ton_step, 1.0, 1.0, 0.05, 0.5], np.full(n, 0.5)])  # :223-231
    v_lo, v_hi = (v0 - 1e-5, v0 + 1e-5) if load_prev else (0.0, 10.0)         # :235-241
    lower = np.concatenate([[v_lo, 0, 0, 0, 0, 0, 0], np.full(n, -30.0)])     # :242-255
    upper = np.concatenate([[v_hi, 20, 10, 50, 50, 1, 40], np.full(n, 30.0)])
    mu = np.zeros(7 + n)
    sig = np.concatenate([np.full(7, np.inf), np.full(n, float(ratePriorWidth))])  # :254
    return x0, lower, upper, mu, sig, J0


def replicate_keys(cells_global, replicates: int) -> np.ndarray:
    """The RNG stream keys of a replicate fit, replicate-major: ``g + r * REPLICATE_KEY_STRIDE`` for replicate ``r``
    of dataset-wide cell ``g`` (replicate 0: ``g``, the one-chain fit's key). The keys are distinct modulo 2^32, which
    is all of a key the sampler's generator sees; ValueError when that cannot be (more than ``MAX_REPLICATES``
    replicates, or with replicates a cell index at or above ``REPLICATE_KEY_STRIDE``)."""
    g = np.asarray(cells_global, np.int64).reshape(-1)
    M = int(replicates)
    if M != replicates or M < 1:
        raise ValueError("replicates must be an integer >= 1")
    if M > MAX_REPLICATES:
        raise ValueError(f"replicates must be at most {MAX_REPLICATES}: a chain's RNG stream key has 32 bits")
    if M > 1 and g.size and (g.min() < 0 or g.max() >= REPLICATE_KEY_STRIDE):
        raise ValueError(f"replicates > 1 needs dataset-wide cell indices below {REPLICATE_KEY_STRIDE}: a chain's RNG "
                         "stream key has 32 bits")
    return np.concatenate([g + r * REPLICATE_KEY_STRIDE for r in range(M)])


@dataclass
class FitResult:
    DatasetName: str
    MCMCresults: List[Dict]
    MCMCplot: List[Dict]
    MCMCchain: List[Dict]
    accept_rate: np.ndarray
    n_evals: int
    elapsed_ms: float
    cell_index: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))   # 0-based, dataset-wide
    final_theta: Optional[np.ndarray] = None   # last chain row per fitted cell (padded), mcmcstat results.theta
    gather_s: float = 0.0                      # parallel.fit_sharded: wall time of the results all-gather
    gather_bytes: int = 0                      # parallel.fit_sharded: bytes every rank receives in it
    local: Optional["FitResult"] = None        # parallel.fit_sharded: this rank's own fit (raw chains, final_theta)
    rows_per_lane_uniform: bool = True         # parallel.fit_sharded: every rank ran the same likelihood variant
    MCMCcheck: Optional[List[Dict]] = None     # fitcheck(lk, fit_result): CHECK_FIELDS per fitted cell
    MCMCsearch: Optional[List[Dict]] = None    # fit(..., presearch=dict(...)): SEARCH_FIELDS per fitted cell
    MCMCdemc: Optional[List[Dict]] = None      # fit(..., demc=dict(...)): DEMC_FIELDS per fitted cell
    MCMCdemczs: Optional[List[Dict]] = None    # fit(..., demczs=dict(...)): DEMCZS_FIELDS per fitted cell
    MCMCtemper: Optional[List[Dict]] = None    # fit(..., temper=R): TEMPER_FIELDS per fitted cell
    MCMCstack: Optional[List[Dict]] = None     # fit(..., stack=nsample): STACK_FIELDS per fitted cell
    MCMClp: Optional[List[Dict]] = None        # fit(..., logpost=True): LP_FIELDS (+ LP_GROUP_FIELDS) per fitted cell
    MCMCess: Optional[List[Dict]] = None       # fit(..., replicates=M, ess=True): ESS_FIELDS per fitted cell
    MCMCrank: Optional[List[Dict]] = None      # fit(..., replicates=M, rank=True): RANK_FIELDS per fitted cell
    MCMCrhat: Optional[List[Dict]] = None      # fit(..., replicates=M): RHAT_FIELDS per fitted cell
    MCMCdens: Optional[List[Dict]] = None      # fit(..., density=True): DENS_FIELDS per fitted cell
    MCMCquant: Optional[List[Dict]] = None     # fit(..., quantiles=probs): QUANT_FIELDS per fitted cell
    MCMCdiag: Optional[List[Dict]] = None      # fit(..., diagnostics=True): DIAG_FIELDS per fitted cell
    MCMCcov: Optional[List[Dict]] = None       # fit(..., covariance=True): COV_FIELDS per fitted cell


@dataclass
class PreviousFit:
    """One ``MCMCresults`` entry of an earlier fit as ``loadPrevious`` keeps it
    (TranscriptionCycleMCMC.m:100-104): the elongation rate and the curation flag."""

    mean_v: Optional[float]
    ApprovedFits: int = 0


def _per_cell(values, c: int):
    """Value for 0-based cell ``c`` of a per-cell input: a mapping keyed by the reference's
    1-based ``cell_index`` (what :func:`load_previous` returns), or a sequence over every cell
    of the dataset (0-based). Missing from a mapping -> None."""
    if values is None:
        return None
    if isinstance(values, Mapping):
        return values.get(c + 1)
    return values[c]


@dataclass
class FitPlan:
    """Per-chain inputs of one fit (TranscriptionCycleMCMC.m:193-255), rows padded to ``ld``."""

    cells: List[int]          # 0-based cell indices that get a chain (skipped cells removed, :196-198)
    x0: np.ndarray
    lower: np.ndarray
    upper: np.ndarray
    prior_mu: np.ndarray
    prior_sig: np.ndarray
    qcov_diag: np.ndarray
    approved: List[int]       # MCMCresults.ApprovedFits per fitted cell (:345-350)
    replicates: int = 1       # chains per cell; the rows are replicate-major: row r * len(cells) + k is cell k's r-th


def _previous(v0, approved, g: int):
    """(skip, v0 of the cell or None, ApprovedFits) for dataset-wide 0-based cell ``g`` (:193-198, :345-350)."""
    prev = _per_cell(v0, g)
    a = 0
    if isinstance(prev, PreviousFit):
        a = int(prev.ApprovedFits)
        prev = prev.mean_v
    if v0 is not None and (prev is None or np.size(prev) != 1 or not np.isfinite(float(prev))):
        return True, None, a
    ap = _per_cell(approved, g)
    if ap is not None:
        a = int(ap)
    return False, (None if v0 is None else float(prev)), a


def kept_cells(cl: Cells, ids: Sequence[int], v0=None, cell_offset: int = 0) -> List[int]:
    """The cells of ``ids`` that get a chain: those with a previous entry when ``v0`` is given
    (:196-198), all of them otherwise -- :func:`plan_fit`'s rule, without drawing anything."""
    return [int(c) for c in ids if not _previous(v0, None, int(cell_offset) + int(c))[0]]


def plan_fit(cl: Cells, ids: Sequence[int], seed: int, ratePriorWidth: float = 50.0, v0=None,
             approved=None, cell_offset: int = 0, replicates: int = 1) -> FitPlan:
    """The parfor body's per-cell setup for the cells ``ids`` (host only, no GPU).

    ``v0`` (loadPrevious, :193-198) and ``approved`` are per-cell inputs read by cell, never by
    position in ``ids``: a mapping keyed by 1-based ``cell_index`` (:194 matches
    ``[MCMCresults.cell_index] == cellNum``) or a sequence over all cells. A ``PreviousFit`` value
    carries both. A cell with no previous entry, or an empty/NaN ``mean_v``, is skipped
    (``continue``, :196-198) and so pruned from the outputs (:359-369). ``ApprovedFits`` is the
    previous fit's when v0 came from one (:345-347) unless ``approved`` overrides it; 0 otherwise
    (:349). ``cell_offset``: the dataset-wide index of ``cl``'s cell 0 (``cl`` holds one shard of a
    larger dataset): x0 and the per-cell inputs are keyed by the dataset-wide index.

    ``replicates``: chains per cell. Replicate 0 of dataset-wide cell ``g`` draws x0 from ``default_rng([seed, g])``
    (what a one-chain fit draws), replicate ``r >= 1`` from ``default_rng([seed, g, r])``; bounds, priors, J0 and a
    hierarchical v0 are the cell's own for every replicate. The rows are replicate-major, so the first
    ``len(cells)`` rows are exactly the one-chain plan."""
    M = int(replicates)
    if M != replicates or M < 1:
        raise ValueError("replicates must be an integer >= 1")
    rows, keep, appr = [], [], []
    for c in ids:
        c = int(c)
        t = cl.cell(c)[0]
        g = int(cell_offset) + c
        skip, vv, a = _previous(v0, approved, g)
        if skip:
            continue
        rows.append(cell_setup(t, np.random.default_rng([int(seed), g]), ratePriorWidth, vv))
        keep.append(c)
        appr.append(a)
    for r in range(1, M):
        for c in keep:
            g = int(cell_offset) + c
            rows.append(cell_setup(cl.cell(c)[0], np.random.default_rng([int(seed), g, r]), ratePriorWidth,
                                   _previous(v0, approved, g)[1]))
    ld = max((len(r[0]) for r in rows), default=7)

    def stack(i, fill):
        out = np.full((len(rows), ld), fill, np.float64)
        for k, r in enumerate(rows):
            out[k, :len(r[i])] = r[i]
        return out

    return FitPlan(keep, stack(0, 0.0), stack(1, -np.inf), stack(2, np.inf), stack(3, 0.0), stack(4, np.inf),
                   stack(5, 1.0), appr, M)


def fit(lk, n_steps: int = 20000, n_burn: int = 10000, ratePriorWidth: float = 50.0, seed: int = 0,
        v0=None, approved=None, thin: int = 0, cells: Optional[Sequence[int]] = None,
        opts: Optional[DramOptions] = None, cell_offset: int = 0, diagnostics: bool = False,
        max_lag: int = 0, covariance: bool = False, quantiles=None, density=None, replicates: int = 1,
        rhat: Optional[bool] = None, ess: bool = False, logpost: bool = False,
        stack: Optional[int] = None, temper=None, swap_every: int = 1, presearch: Optional[Mapping] = None,
        demc: Optional[Mapping] = None, rank=False, demczs: Optional[Mapping] = None) -> FitResult:
    """``TranscriptionCycleMCMC`` for one dataset on the GPU: one DRAM chain per cell.

    ``lk``: a ``Likelihood`` holding the (truncated) cells. ``v0``: the previous fit of a
    hierarchical run (loadPrevious): ``load_previous(path)`` (cell_index -> PreviousFit), a
    mapping cell_index -> mean_v, or a sequence of rates over ALL cells (None/NaN = no entry).
    Cells without an entry are skipped (``continue``, :196-198) and pruned from the outputs
    (:359-369); see :func:`plan_fit`. ``thin``: keep every thin-th raw chain row in ``MCMCchain``
    (the reference keeps all rows from n_burn, :276-283 -- ~193 MB/cell at 200k steps; thin=1
    reproduces that). ``cells``: fit only these cell indices (a shard).

    Everything random is keyed by the cell index -- x0 by ``default_rng([seed, cell])``, the chain
    by RNG stream ``cell`` -- so fitting a subset of the cells (one GPU's shard,
    :func:`parallel.fit_sharded`) reproduces those cells' results of the full fit bit for bit.
    ``cell_offset``: ``lk`` holds only a contiguous block of a larger dataset, starting at this
    dataset-wide cell index; keys, x0, per-cell inputs and ``cell_index`` use the dataset-wide index
    (a rank that loaded only its own shard reproduces the one-GPU fit of the whole dataset).

    ``diagnostics``: also ``MCMCdiag``, one dict of ``DIAG_FIELDS`` per fitted cell: the Monte-Carlo
    error, the integrated autocorrelation time and Geweke's p of every parameter and of s2, over the
    rows ``MCMCchain`` keeps (needs ``thin >= 1``), reduced on the device (:func:`diag_entry`).

    ``covariance``: also ``MCMCcov``, one dict of ``COV_FIELDS`` per fitted cell: the posterior mean
    ``[P]``, covariance and correlation ``[P, P]`` (``P = 7 + N``; MATLAB's ``cov(chain)`` and
    ``corrcoef(chain)``) of the rows ``MCMCchain`` keeps (needs ``thin >= 1`` and 2 such rows), reduced on
    the device.

    ``quantiles``: a sequence of 1 to 16 probabilities: also ``MCMCquant``, one dict of ``QUANT_FIELDS`` per
    fitted cell: the exact quantiles (mcmcstat's ``plims``: median, credible intervals) of every parameter and
    of s2 over the rows ``MCMCchain`` keeps (needs ``thin >= 1``), selected on the device (:func:`quant_entry`).

    ``density``: ``True`` or a dict of ``n_grid`` / ``n_bins`` / ``bw_scale``: also ``MCMCdens``, one dict of
    ``DENS_FIELDS`` per fitted cell: the marginal density (mcmcstat's ``density.m``) and histogram of every
    parameter and of s2 over the rows ``MCMCchain`` keeps (needs ``thin >= 1`` and 2 such rows), reduced on the
    device (:func:`dens_entry`): what ``ApproveMCMCResults`` draws with ``histogram`` from the raw chains.

    ``replicates``: M chains per cell instead of one, from different starts (:func:`plan_fit`); replicate ``r >= 1``
    of cell ``g`` runs on RNG stream ``g + r * 2**24`` (:func:`replicate_keys`; the generator sees a key's low 32 bits,
    so at most 256 replicates and cell indices below 2**24). The chains are ordered replicate-major, and the engines and
    reductions do not depend on a chain's position: ``MCMCresults``, ``MCMCplot``, ``MCMCchain``, ``accept_rate``,
    ``final_theta`` and the four optional per-cell lists are replicate 0's, bit for bit those of ``replicates=1``
    (``n_evals`` counts every replicate). ``rhat`` (default: ``replicates > 1``): also ``MCMCrhat``, one dict of
    ``RHAT_FIELDS`` per fitted cell: Gelman-Rubin's classic and split potential scale reduction factor and the pooled
    posterior mean and standard deviation of every parameter and of s2 across the cell's replicates, over the rows
    ``MCMCchain`` keeps (needs ``thin >= 1`` and 2 such rows), reduced on the device (:func:`rhat_entry`).
    ``rhat=True`` with one replicate gives the split factor alone (the classic one is NaN). With ``thin >= 1`` the
    kept rows of every replicate are copied to the host, M times the one-chain fit's copy, though ``MCMCchain`` keeps
    replicate 0's alone (``tci_dram_outputs.chain`` is all chains or none).

    ``ess`` (needs ``MCMCrhat``, i.e. replicates or ``rhat=True``): also ``MCMCess``, one dict of ``ESS_FIELDS`` per
    fitted cell: the multi-chain effective sample size (BDA3 11.5) and autocorrelation time, classic and split, the
    lags summed and the pooled mean's Monte-Carlo standard error, over the same rows and reduced on the device
    (:func:`ess_entry`); ``max_lag`` caps its lags as it caps the diagnostics'. Nothing else in the result changes.

    ``rank`` (needs ``MCMCrhat`` as ``ess`` does): ``True`` or a dict of ``probs`` / ``tail``: also ``MCMCrank``, one
    dict of ``RANK_FIELDS`` per fitted cell: the rank-normalised split R-hat (bulk, folded and their maximum), bulk and
    tail ESS and the pooled quantiles of the cell's replicates (``Likelihood.chainrank``; :func:`rank_entry`), from the
    device chain through ``tci_dram_run_rank``; with ``logpost`` or ``temper`` from the kept rows through
    ``tci_chainrank``, the same bits. With ``demc`` the same values join every ``MCMCdemc`` entry.

    ``logpost``: also ``MCMClp``, one dict of ``LP_FIELDS`` per fitted cell: the sum-of-squares trace (mcmcstat's
    ``sschain``) and the log-posterior trace of the rows ``MCMCchain`` keeps (needs ``thin >= 1``), the best sample (a
    posterior-mode estimate) and DIC, all on the device (:func:`lp_entry`). With ``replicates=M`` the entry holds every
    replicate's values and ``LP_GROUP_FIELDS``: R-hat, ESS and MCSE of ``lp`` across the replicates (the ``lp__``
    diagnostic), ``ss_gap`` and ``best_replicate``: whether replicates that disagree sit at different SS levels. The
    priors :func:`plan_fit` builds always pass the check ``dram_run(..., logpost=True)`` makes on them (a
    ``ratePriorWidth`` that is NaN or <= 0 does not: such a fit runs without ``logpost`` and is refused with it).

    ``stack``: a sample count in [32, 4096]: also ``MCMCstack``, one dict of ``STACK_FIELDS`` per fitted cell (needs
    ``thin >= 1`` and at least 32 kept post-burn-in rows): the PSIS-LOO expected log predictive density and Pareto k
    of every replicate over :func:`predict_rows` of its kept rows, and the weights across the cell's replicates that
    maximise the stacked leave-one-out density (``Likelihood.loocheck``, on the device; :func:`stack_entries`):
    the estimate for replicates that do not mix. ``replicates=1`` gives the LOO values alone, with weight 1. Nothing
    else in the result changes.

    ``temper``: parallel tempering (include/tci.h, ``tci_dram_run_tempered``). An integer ``R``: a ladder of ``R`` rungs
    per (cell, replicate) at :func:`temper_ladder` of the cell's ``P = 7 + N``; or a sequence of inverse temperatures,
    strictly decreasing from 1, used for every cell. Neighbouring rungs exchange states after every ``swap_every``-th
    adaptation window. Row layout: the fit runs ``M * R`` chains per cell, chain ``(q * M + r) * K + k`` being rung ``q``
    of replicate ``r`` of fitted cell ``k`` (``K`` cells): the ``M * K`` cold rungs (``beta = 1``) come first in
    today's replicate-major order and the hot rungs follow; they start where replicates ``M .. M * R - 1`` of
    :func:`plan_fit` start and run on those replicates' RNG streams (so ``M * R <= 256``). The reductions and groups
    apply to the cold rungs alone: every other field of the result is the cold rungs', computed as without tempering.
    ``MCMCtemper`` holds one dict of ``TEMPER_FIELDS`` per fitted cell. ``temper=1`` or its absence is the untempered
    fit, bit for bit.

    ``presearch``: a dict of ``n_pop`` / ``n_gen`` / ``F`` / ``CR`` (any may be left out: :func:`modesearch`'s defaults):
    a mode search (include/tci.h, ``tci_modesearch``) runs first on :func:`search_population` of every fitted cell, which
    holds every replicate's usual start, and replicate ``r`` of a cell starts from the ``r``-th best final member (by
    ``f``, ties by index; needs ``replicates <= n_pop``); the rungs of a tempered replicate start from their replicate's
    member. Everything else is unchanged. ``MCMCsearch`` holds one dict of ``SEARCH_FIELDS`` per fitted cell.
    ``presearch=None`` (the default) takes no new code path.

    ``demc``: a dict with keys among ``DEMC_KEYS`` (``n_pop`` and ``n_gen`` default to :func:`demc`'s): the cells are
    sampled by the DE-MC population sampler (include/tci.h, ``tci_demc_run``) instead of DRAM; ``n_steps`` and ``opts``
    are not used, ``n_burn`` counts generations and ``thin >= 1`` is needed. Every field of the result comes from the
    kept rows of generations ``>= n_burn`` of all members pooled (``MCMCchain``'s ``s2chain`` alone holds every kept
    row, as the reference's is not sliced by n_burn; ``final_theta``: member 0's last state;
    ``accept_rate``: the members' mean), and ``MCMCdemc`` holds one dict of ``DEMC_FIELDS`` per fitted cell, R-hat and
    the multi-chain ESS across the members reduced on the device. With ``presearch`` the population starts from the
    search's final one (its ``n_pop`` is the sampler's). It cannot be combined with ``temper`` or ``replicates``, which
    are DRAM's, nor with the DRAM reductions. ``demc=None`` (the default) is today's fit bit for bit.

    ``demczs``: a dict with keys among ``DEMCZS_KEYS`` (defaults: :func:`demczs`'s): the cells are sampled by the
    DE-MC(zs) sampler (include/tci.h, ``tci_demczs_run``): ``n_pop`` chains per cell (default 4) that propose from an
    archive of past states. Everything said of ``demc`` holds, the chains taking the members' place; ``MCMCdemczs`` holds
    one dict of ``DEMCZS_FIELDS`` per fitted cell. With ``presearch`` the search runs ``m0`` members, its final
    population is the archive and the chains start at its best members. ``snooker_rate`` is the share of snooker moves
    among the first ``ZS_FIT_LOG_ROWS`` (1,024) generations, the ones the fit logs, not of the whole run. Rows kept while the archive is young are
    burn-in: ``n_burn`` is the caller's to set. Exclusive with ``demc`` too. ``demczs=None`` (the default) is today's
    fit bit for bit."""
    M = int(replicates)
    if demczs is not None:
        if demc is not None:
            raise ValueError("demczs and demc are two samplers: give one")
        if M != 1 or _temper_arg(temper)[1] > 1:
            raise ValueError("demczs is a sampler of its own: it cannot be combined with temper or replicates (its "
                             "chains are the cell's chains)")
        want_rank = rank is not None and rank is not False
        if want_rank and not isinstance(rank, (bool, Mapping)):
            raise ValueError("rank must be True or a dict with keys among ('probs', 'tail')")
        if diagnostics or covariance or quantiles is not None or density or logpost or stack is not None or rhat or ess:
            raise ValueError("demczs does not take the DRAM reductions (diagnostics, covariance, quantiles, density, "
                             "rhat, ess, logpost, stack): MCMCdemczs holds R-hat and ESS across the chains")
        return _fit_demc(lk, demczs, n_burn, ratePriorWidth, seed, v0, approved, thin, cells, cell_offset, presearch,
                         max_lag, rank if want_rank else False, zs=True)
    ps = _presearch_arg(presearch, M)
    betas, R = _temper_arg(temper)
    if demc is not None:
        if M != 1 or R > 1:
            raise ValueError("demc is a population sampler of its own: it cannot be combined with temper or replicates "
                             "(its members are the cell's chains)")
        want_rank = rank is not None and rank is not False
        if want_rank and not isinstance(rank, (bool, Mapping)):
            raise ValueError("rank must be True or a dict with keys among ('probs', 'tail')")
        if diagnostics or covariance or quantiles is not None or density or logpost or stack is not None or rhat or ess:
            raise ValueError("demc does not take the DRAM reductions (diagnostics, covariance, quantiles, density, rhat, "
                             "ess, logpost, stack): MCMCdemc holds R-hat and ESS across the members")
        return _fit_demc(lk, demc, n_burn, ratePriorWidth, seed, v0, approved, thin, cells, cell_offset, presearch, max_lag,
                         rank if want_rank else False)
    if R > 1 and (isinstance(swap_every, bool) or int(swap_every) != swap_every or int(swap_every) < 0):
        raise ValueError("swap_every must be an integer >= 0")
    if M != replicates or M < 1:
        raise ValueError("replicates must be an integer >= 1")
    want_rhat = M > 1 if rhat is None else bool(rhat)
    if want_rhat and int(thin) < 1:
        raise ValueError("MCMCrhat is reduced from the kept rows: replicates > 1 (or rhat=True) needs thin >= 1; "
                         "pass rhat=False to run the replicates without it")
    if ess and not want_rhat:
        raise ValueError("MCMCess is reduced with MCMCrhat: ess=True needs replicates > 1 or rhat=True")
    want_rank = rank is not None and rank is not False
    if want_rank and not want_rhat:
        raise ValueError("MCMCrank is reduced with MCMCrhat: rank needs replicates > 1 or rhat=True")
    if want_rank and (not isinstance(rank, (bool, Mapping)) or (isinstance(rank, Mapping) and set(rank) - {"probs", "tail"})):
        raise ValueError("rank must be True or a dict with keys among ('probs', 'tail')")
    rank_kw = dict(rank) if isinstance(rank, Mapping) else {}
    rank_host = want_rank and (logpost or R > 1)   # no entry point takes rank with these: from the kept rows instead
    if logpost and int(thin) < 1:
        raise ValueError("MCMClp is reduced from the kept rows: logpost=True needs thin >= 1")
    if stack is not None:
        if isinstance(stack, bool) or int(stack) != stack or not 32 <= int(stack) <= 4096:
            raise ValueError("stack must be an integer sample count in [32, 4096]")
        if int(thin) < 1:
            raise ValueError("MCMCstack is reduced from the kept rows: stack=nsample needs thin >= 1")
    cl: Cells = lk.cells
    ids = list(range(cl.n_cells)) if cells is None else [int(c) for c in cells]
    off = int(cell_offset)
    if M * R > MAX_REPLICATES:
        raise ValueError(f"replicates * temper must be at most {MAX_REPLICATES}: a chain's RNG stream key has 32 bits")
    plan = plan_fit(cl, ids, seed, ratePriorWidth, v0, approved, cell_offset=off, replicates=M * R)
    keep = plan.cells
    K = len(keep)
    MK = M * K
    if not keep:
        return FitResult(cl.name, [], [], [], np.zeros(0), 0, 0.0)
    # a private copy: the caller's options object is never modified
    o = dataclasses.replace(opts) if opts is not None else DramOptions()
    o.n_steps, o.burnintime, o.stats_from, o.thin = int(n_steps), int(n_burn), int(max(n_burn, 1)), int(thin)
    o.seed = int(seed) * 1000003 + 20201028
    keys = replicate_keys(np.array(keep, np.int64) + off, M * R)
    searched = None
    if ps is not None:
        sr, sp = modesearch(lk, seed=seed, cells=keep, v0=v0, cell_offset=off, ratePriorWidth=ratePriorWidth, **ps)
        if sp.cells != keep:   # row k of the search must be fitted cell k
            raise RuntimeError(f"presearch searched cells {sp.cells}, the fit keeps {keep}")
        searched = [search_entry(sr, k, int(cl.lengths[c]), off + c + 1) for k, c in enumerate(keep)]
        for k, c in enumerate(keep):
            P = 7 + int(cl.lengths[c])
            order = search_order(sr.f[k])
            for q in range(R):
                for r in range(M):
                    plan.x0[(q * M + r) * K + k, :P] = sr.pop[k, order[r], :P]
    tk = {}
    if R > 1:
        tk = temper_layout([int(cl.lengths[c]) for c in keep], M, R, betas)
        tk["swap_every"] = int(swap_every)
    cold_group = np.concatenate([np.tile(np.arange(K, dtype=np.int32), M), np.full(MK * (R - 1), -1, np.int32)])
    res = dram_run(lk, np.tile(np.array(keep, np.int32), M * R), plan.x0, plan.lower, plan.upper, plan.prior_mu,
                   plan.prior_sig, plan.qcov_diag, 1.0, o, chain_keys=keys, **tk,
                   **(dict(group=cold_group) if want_rhat else {}),
                   **(dict(ess=True) if ess and R == 1 else {}),
                   **(dict(rank=rank_kw or True) if want_rank and not rank_host else {}),
                   **(dict(logpost=True) if logpost and R == 1 else {}),
                   **(dict(stats=True) if diagnostics else {}),
                   **(dict(max_lag=max_lag) if ess or diagnostics or want_rank else {}),
                   **(dict(cov=True) if covariance else {}),
                   **(dict(quant=quantiles) if quantiles is not None else {}),
                   **(dict(dens=density) if density is not None and density is not False else {}))
    tempers = None
    if R > 1:
        tempers = [temper_entry(res, k, K, M, R, off + c + 1) for k, c in enumerate(keep)]
        # the tempered entry point has no effective sample size or log-posterior reduction: those of the cold rungs
        # from their kept rows on the host, through the same kernels
        if ess or logpost or rank_host:
            if res.chain is None:
                raise ValueError("ess and logpost of a tempered fit are reduced from the kept rows: thin >= 1")
            sel = 1 + int(thin) * np.arange(res.chain.shape[0]) >= max(n_burn, 1)
            cold_chain, cold_s2 = res.chain[sel][:, :MK], res.s2chain[sel][:, :MK]
            cid = np.tile(np.array(keep, np.int32), M)
            if ess:
                res.ess = lk.chainess(cold_chain, cold_s2, npar=7 + lk.cells.lengths[cid], group=cold_group[:MK],
                                      max_lag=max_lag)
            if logpost:
                res.lp = lk.chainlp(cold_chain, cold_s2, cid, plan.prior_mu[:MK], plan.prior_sig[:MK])
            if rank_host:
                res.rank = lk.chainrank(cold_chain, cold_s2, npar=7 + lk.cells.lengths[cid], group=cold_group[:MK],
                                        max_lag=max_lag, **rank_kw)
        # every per-chain field below is read by cell and replicate: the cold rungs'
        res.mean, res.accept_rate = res.mean[:MK], res.accept_rate[:MK]
        if res.chain is not None:
            res.chain, res.s2chain = res.chain[:, :MK], res.s2chain[:, :MK]
    # forward model at the means on the raw times (:307-309)
    ms2, pp7 = lk.forward(res.mean[:K], np.array(keep, np.int32), grid="raw")
    results, plots, chains = [], [], []
    for k, c in enumerate(keep):
        t, m, p = cl.cell(c)
        n = len(t)
        mean, std = res.mean[k, :7 + n], res.std[k, :7 + n]
        r = {}
        for name in ("v", "ton", "A", "tau", "MS2_basal", "PP7_basal", "R"):
            r["mean_" + name] = float(mean[THETA_INDEX[name]])
            r["sigma_" + name] = float(std[THETA_INDEX[name]])
        r["mean_dR"], r["sigma_dR"] = mean[7:].copy(), std[7:].copy()
        r["mean_sigma"], r["sigma_sigma"] = float(res.sigma_mean[k]), float(res.sigma_std[k])
        r["cell_index"] = off + c + 1                                         # :343 (1-based)
        r["ApprovedFits"] = plan.approved[k]                                  # :345-350
        results.append({f: r[f] for f in RESULT_FIELDS})
        plots.append({"t_plot": t.copy(), "MS2_plot": m.copy(), "PP7_plot": p.copy(),
                      "simMS2": ms2[k, :n].copy(), "simPP7": pp7[k, :n].copy()})
        ch = {}
        if res.chain is not None:
            # rows kept: 1, 1+thin, ...; the reference stores chain(n_burn:end, :) (:276-283)
            rows_idx = 1 + thin * np.arange(res.chain.shape[0])
            sel = rows_idx >= max(n_burn, 1)
            th = res.chain[sel, k, :7 + n]
            for name in ("v", "ton", "A", "tau", "MS2_basal", "PP7_basal", "R"):
                ch[name + "_chain"] = th[:, THETA_INDEX[name]].copy()
            ch["dR_chain"] = th[:, 7:].copy()
            ch["s2chain"] = res.s2chain[:, k].copy()  # s2chain is not sliced by n_burn (:323)
        chains.append(ch)
    diag = None
    if diagnostics:
        diag = [diag_entry(res.stats, k, int(cl.lengths[c]), off + c + 1) for k, c in enumerate(keep)]
    cov = None
    if covariance:
        cov = [cov_entry(res.cov, k, int(cl.lengths[c]), off + c + 1) for k, c in enumerate(keep)]
    quant = None
    if quantiles is not None:
        quant = [quant_entry(res.quant, k, int(cl.lengths[c]), off + c + 1) for k, c in enumerate(keep)]
    dens = None
    if res.dens is not None:
        dens = [dens_entry(res.dens, k, int(cl.lengths[c]), off + c + 1) for k, c in enumerate(keep)]
    rh = None
    if res.rhat is not None:
        rh = [rhat_entry(res.rhat, k, int(cl.lengths[c]), off + c + 1, res.mean[k::K], res.accept_rate[k::K])
              for k, c in enumerate(keep)]
    es = None
    if res.ess is not None:
        es = [ess_entry(res.ess, k, int(cl.lengths[c]), off + c + 1, M) for k, c in enumerate(keep)]
    if rank_host and R == 1:
        sel = 1 + int(thin) * np.arange(res.chain.shape[0]) >= max(n_burn, 1)
        res.rank = lk.chainrank(res.chain[sel], res.s2chain[sel], npar=7 + cl.lengths[np.tile(np.array(keep), M)],
                                group=cold_group, max_lag=max_lag, **rank_kw)
    rk = None
    if res.rank is not None:
        rk = [rank_entry(res.rank, k, int(cl.lengths[c]), off + c + 1, M) for k, c in enumerate(keep)]
    lps = None
    if res.lp is not None:
        grp = lp_group_stats(lk, res.lp, K, M, max_lag) if M > 1 else None
        lps = [lp_entry(res.lp, k, int(cl.lengths[c]), off + c + 1, K, M, grp) for k, c in enumerate(keep)]
    stk = None
    if stack is not None:
        rows_idx = 1 + int(thin) * np.arange(res.chain.shape[0])
        stk = stack_entries(lk, res.chain[rows_idx >= max(n_burn, 1)], res.s2chain, res.mean, keep, M, int(stack), off)
    return FitResult(cl.name, results, plots, chains, res.accept_rate[:K].copy(), int(res.n_evals.sum()),
                     res.elapsed_ms, np.array(keep, np.int64) + off, res.final_theta[:K].copy(), MCMClp=lps, MCMCess=es,
                     MCMCrank=rk, MCMCrhat=rh, MCMCstack=stk, MCMCtemper=tempers, MCMCsearch=searched,
                     MCMCdens=dens, MCMCquant=quant, MCMCdiag=diag, MCMCcov=cov)


def _presearch_arg(presearch, replicates: int):
    """``fit``'s ``presearch`` as keyword arguments of :func:`modesearch`, or None."""
    if presearch is None:
        return None
    if not isinstance(presearch, Mapping):
        raise ValueError(f"presearch must be a dict with keys among {PRESEARCH_KEYS}")
    bad = sorted(set(presearch) - set(PRESEARCH_KEYS))
    if bad:
        raise ValueError(f"presearch has unknown keys {bad}: the keys are {PRESEARCH_KEYS}")
    ps = dict(presearch)
    n_pop = ps.setdefault("n_pop", 64)
    if isinstance(n_pop, bool) or int(n_pop) != n_pop or not 4 <= int(n_pop) <= 4096:
        raise ValueError("presearch n_pop must be an integer in [4, 4096]")
    if int(replicates) > int(n_pop):
        raise ValueError("presearch starts replicate r from the r-th best member: replicates must be <= n_pop")
    n_gen = ps.get("n_gen", 0)
    if isinstance(n_gen, bool) or int(n_gen) != n_gen or int(n_gen) < 0:
        raise ValueError("presearch n_gen must be an integer >= 0")
    return ps


@dataclass
class SearchPlan:
    """The initial population of a mode search (:func:`search_population`): ``pop0`` ``[K, n_pop, ld]`` for the ``K``
    cells ``cells`` (0-based, skipped cells removed) with their bounds and priors ``[K, ld]``."""

    cells: List[int]
    pop0: np.ndarray
    lower: np.ndarray
    upper: np.ndarray
    prior_mu: np.ndarray
    prior_sig: np.ndarray


def search_population(cl: Cells, ids: Sequence[int], seed: int, n_pop: int, ratePriorWidth: float = 50.0, v0=None,
                      approved=None, cell_offset: int = 0) -> SearchPlan:
    """The initial population of the mode search for the cells ``ids`` (host only): member ``i`` of a cell is the x0 of
    replicate ``i`` of :func:`plan_fit` (member 0 from ``default_rng([seed, g])``, member ``i >= 1`` from
    ``default_rng([seed, g, i])``, ``g`` the dataset-wide cell index), so the population holds every replicate's start
    of a fit of up to ``n_pop`` replicates. Bounds, priors and a hierarchical ``v0`` are :func:`plan_fit`'s."""
    n_pop = int(n_pop)
    plan = plan_fit(cl, ids, seed, ratePriorWidth, v0, approved, cell_offset=cell_offset, replicates=n_pop)
    K = len(plan.cells)
    ld = plan.x0.shape[1]
    pop0 = np.ascontiguousarray(plan.x0.reshape(n_pop, K, ld).transpose(1, 0, 2))
    return SearchPlan(plan.cells, pop0, plan.lower[:K].copy(), plan.upper[:K].copy(), plan.prior_mu[:K].copy(),
                      plan.prior_sig[:K].copy())


def modesearch(lk, n_pop: int = 64, n_gen: int = 500, seed: int = 0, cells: Optional[Sequence[int]] = None, v0=None,
               cell_offset: int = 0, ratePriorWidth: float = 50.0, F: float = 0.5, CR: float = 0.9, s2=1.0,
               approved=None):
    """A mode search (``Likelihood.modesearch``) from :func:`search_population` of the cells ``cells`` (default: all) of
    ``lk``. Everything random is keyed by the dataset-wide cell index (the population by ``default_rng``, the search by
    RNG stream ``cell_offset + cell``) and seeded as :func:`fit` seeds its sampler, so a shard reproduces its cells of
    the full search bit for bit. Returns ``(ModeSearch, SearchPlan)``; row ``k`` of either is cell ``plan.cells[k]``."""
    cl: Cells = lk.cells
    ids = list(range(cl.n_cells)) if cells is None else [int(c) for c in cells]
    sp = search_population(cl, ids, seed, n_pop, ratePriorWidth, v0, approved, cell_offset)
    if not sp.cells:
        return ModeSearch.empty(0, int(n_pop), sp.pop0.shape[2], int(n_gen)), sp
    res = lk.modesearch(sp.pop0, np.array(sp.cells, np.int32), sp.lower, sp.upper, sp.prior_mu, sp.prior_sig, s2=s2,
                        n_gen=n_gen, F=F, CR=CR, seed=int(seed) * 1000003 + 20201028,
                        keys=np.array(sp.cells, np.int64) + int(cell_offset))
    return res, sp


def _demc_arg(demc):
    """``fit``'s ``demc`` as keyword arguments of :func:`demc`."""
    if not isinstance(demc, Mapping):
        raise ValueError(f"demc must be a dict with keys among {DEMC_KEYS}")
    bad = sorted(set(demc) - set(DEMC_KEYS))
    if bad:
        raise ValueError(f"demc has unknown keys {bad}: the keys are {DEMC_KEYS}")
    d = dict(demc)
    n_pop = d.setdefault("n_pop", 64)
    if isinstance(n_pop, bool) or int(n_pop) != n_pop or not 4 <= int(n_pop) <= 4096:
        raise ValueError("demc n_pop must be an integer in [4, 4096]")
    n_gen = d.setdefault("n_gen", 1000)
    if isinstance(n_gen, bool) or int(n_gen) != n_gen or int(n_gen) < 1:
        raise ValueError("demc n_gen must be an integer >= 1")
    return d


def demc_jitter(cl: Cells, ids: Sequence[int], ratePriorWidth: float = 50.0, v0=None, approved=None,
                cell_offset: int = 0) -> np.ndarray:
    """The default jitter half-width of :func:`demc`, ``[K, ld]``: ``1e-3 * sqrt(qcov_diag)`` of :func:`cell_setup`
    (padding 0). A starting value, not a measured optimum."""
    plan = plan_fit(cl, ids, 0, ratePriorWidth, v0, approved, cell_offset=cell_offset)
    jit = 1e-3 * np.sqrt(plan.qcov_diag)
    for k, c in enumerate(plan.cells):
        jit[k, 7 + int(cl.lengths[c]):] = 0.0
    return jit


def demc(lk, n_pop: int = 64, n_gen: int = 1000, thin: int = 1, n_burn: int = 0, seed: int = 0,
         cells: Optional[Sequence[int]] = None, v0=None, presearch=None, cell_offset: int = 0,
         ratePriorWidth: float = 50.0, jitter=None, CR: float = 0.2, gamma0: float = 0.0, jump_every: int = 10,
         updatesigma: bool = True, sigma2_0=1.0, rhat: bool = True, ess: bool = True, max_lag: int = 0,
         log_rows: int = 0, approved=None, rank=False):
    """A DE-MC run (``Likelihood.demc``; include/tci.h, ``tci_demc_run``) of the cells ``cells`` (default: all) of
    ``lk`` from :func:`search_population`, or from the final population of a mode search when ``presearch`` is given: a
    dict of ``n_gen`` / ``F`` / ``CR`` for :func:`modesearch` (run here with the same ``n_pop`` and ``seed``), or the
    ``(ModeSearch, SearchPlan)`` such a call returned. Everything random is keyed by the dataset-wide cell index (the
    population by ``default_rng``, the run by RNG stream ``cell_offset + cell``) and seeded as :func:`fit` seeds its
    sampler, so a shard reproduces its cells of the full run bit for bit. ``jitter``: ``[K, ld]`` half-widths, a scalar
    factor on :func:`demc_jitter`'s default, or None. ``n_burn``: the reductions (``rhat`` / ``ess``, across a cell's
    members) use the kept rows of generations ``>= n_burn``; ``rank``: ``True`` or a dict of ``probs`` / ``tail``: the rank
    diagnostics and pooled quantiles of those rows too (``Demc.rank``, as ``Likelihood.chainrank`` gives). Returns
    ``(Demc, SearchPlan)``; row ``k`` of either is cell
    ``plan.cells[k]``."""
    cl: Cells = lk.cells
    ids = list(range(cl.n_cells)) if cells is None else [int(c) for c in cells]
    if isinstance(presearch, tuple):
        sr, sp = presearch
        if sr.pop.shape[1] != int(n_pop):
            raise ValueError("the mode search's n_pop is not the sampler's")
        pop0 = sr.pop
    elif presearch is not None:
        if not isinstance(presearch, Mapping) or set(presearch) - {"n_gen", "F", "CR"}:
            raise ValueError("presearch must be a dict with keys among ('n_gen', 'F', 'CR') or a modesearch result")
        sr, sp = modesearch(lk, n_pop=n_pop, seed=seed, cells=ids, v0=v0, cell_offset=cell_offset,
                            ratePriorWidth=ratePriorWidth, approved=approved, **presearch)
        pop0 = sr.pop
    else:
        sp = search_population(cl, ids, seed, n_pop, ratePriorWidth, v0, approved, cell_offset)
        pop0 = sp.pop0
    if not sp.cells:
        return Demc.empty(0, int(n_pop), sp.pop0.shape[2], int(n_gen), int(thin), 0), sp
    jit = jitter
    if jit is None or np.ndim(jit) == 0:
        base = demc_jitter(cl, sp.cells, ratePriorWidth, v0, approved, cell_offset)
        jit = base if jit is None else float(jit) * base
    res = lk.demc(pop0, np.array(sp.cells, np.int32), sp.lower, sp.upper, sp.prior_mu, sp.prior_sig, jit,
                  sigma2_0=sigma2_0, n_gen=n_gen, thin=thin, jump_every=jump_every, CR=CR, gamma0=gamma0,
                  updatesigma=updatesigma, seed=int(seed) * 1000003 + 20201028,
                  keys=np.array(sp.cells, np.int64) + int(cell_offset), stats_from=n_burn, rhat=rhat, ess=ess,
                  max_lag=max_lag, log_rows=log_rows, rank=rank)
    return res, sp


def demc_entry(res: Demc, k: int, n: int, cell_index: int) -> Dict:
    """One ``MCMCdemc`` entry (``DEMC_FIELDS``) from selected cell ``k`` of ``res``, a cell of ``n`` points: per member
    ``accept_rate``, ``n_oob`` and ``n_evals``; ``rhat_max`` / ``ess_min``: the largest classic R-hat and the least
    multi-chain ESS over the cell's parameters and s2 (NaN without the reduction)."""
    P = 7 + n
    rm = em = float("nan")
    if res.rhat is not None:
        rm = float(np.nanmax(np.append(res.rhat.rhat[k, :P], res.rhat.s2_rhat[k])))
    if res.ess is not None:
        em = float(np.nanmin(np.append(res.ess.ess[k, :P], res.ess.s2_ess[k])))
    d = dict(accept_rate=res.accept_rate[k].copy(), n_oob=res.n_oob[k].copy(), rhat_max=rm, ess_min=em,
             n_pop=int(res.pop.shape[1]), n_gen=int(res.n_gen), n_evals=res.n_evals[k].copy(), cell_index=int(cell_index))
    return {f: d[f] for f in DEMC_FIELDS}


def _fit_demc(lk, demc_arg, n_burn, ratePriorWidth, seed, v0, approved, thin, cells, cell_offset, presearch, max_lag,
              rank=False, zs=False):
    """:func:`fit` with the DE-MC sampler, or with ``zs`` the DE-MC(zs) sampler: every result field from the kept rows of
    all members (chains) pooled."""
    name = "demczs" if zs else "demc"
    kw = _demczs_arg(demc_arg) if zs else _demc_arg(demc_arg)
    if int(thin) < 1:
        raise ValueError(f"a DE-MC fit is reduced from the kept rows: {name} needs thin >= 1")
    n_gen, n_pop = int(kw["n_gen"]), int(kw["n_pop"])
    if n_gen // int(thin) + 1 - -(-int(n_burn) // int(thin)) < 2:
        raise ValueError(f"{name} needs at least 2 kept generations at or past n_burn")
    cl: Cells = lk.cells
    off = int(cell_offset)
    ids = list(range(cl.n_cells)) if cells is None else [int(c) for c in cells]
    keep = kept_cells(cl, ids, v0, off)
    if not keep:
        return FitResult(cl.name, [], [], [], np.zeros(0), 0, 0.0)
    ps = None
    searched = None
    if presearch is not None:
        n_search = n_pop      # the search's members: the population, or with zs the starting archive
        if zs:
            n_search = kw["m0"] = int(kw.get("m0") or demczs_m0(cl, keep))
        pk = _presearch_arg({**presearch, "n_pop": presearch.get("n_pop", n_search)}, 1)
        if int(pk.pop("n_pop")) != n_search:
            raise ValueError("presearch n_pop must be the sampler's " + ("m0" if zs else "n_pop"))
        ps = modesearch(lk, n_pop=n_search, seed=seed, cells=keep, v0=v0, cell_offset=off, ratePriorWidth=ratePriorWidth,
                        approved=approved, **pk)
        searched = [search_entry(ps[0], k, int(cl.lengths[c]), off + c + 1) for k, c in enumerate(keep)]
    res, sp = (demczs if zs else demc)(lk, thin=int(thin), n_burn=int(n_burn), seed=seed, cells=keep, v0=v0, presearch=ps,
                                       cell_offset=off, ratePriorWidth=ratePriorWidth, max_lag=max_lag, approved=approved,
                                       rank=rank, **({"log_rows": min(n_gen, ZS_FIT_LOG_ROWS)} if zs else {}), **kw)
    if sp.cells != keep:
        raise RuntimeError(f"{name} sampled cells {sp.cells}, the fit keeps {keep}")
    K = len(keep)
    ld = res.pop.shape[2]
    sel = int(thin) * np.arange(res.chain.shape[0]) >= int(n_burn)
    chain = res.chain[sel].reshape(-1, K, n_pop, ld)         # [rows, cell, member, ld]
    s2 = res.s2chain.reshape(-1, K, n_pop)                   # s2chain is not sliced by n_burn (:323)
    mean = np.zeros((K, ld))
    for k, c in enumerate(keep):
        P = 7 + int(cl.lengths[c])
        mean[k, :P] = chain[:, k, :, :P].reshape(-1, P).mean(axis=0)
    ms2, pp7 = lk.forward(mean, np.array(keep, np.int32), grid="raw")
    results, plots, chains, entries = [], [], [], []
    for k, c in enumerate(keep):
        t, m, p = cl.cell(c)
        n = len(t)
        th = chain[:, k, :, :7 + n].reshape(-1, 7 + n)       # the members of a row side by side, rows ascending
        std = th.std(axis=0)
        r = {}
        for name in _SCALARS:
            r["mean_" + name] = float(mean[k, THETA_INDEX[name]])
            r["sigma_" + name] = float(std[THETA_INDEX[name]])
        r["mean_dR"], r["sigma_dR"] = mean[k, 7:7 + n].copy(), std[7:].copy()
        sq = s2[:, k].reshape(-1)
        sq_sel = s2[sel, k].reshape(-1)                      # the summaries: generations >= n_burn, as every other one
        r["mean_sigma"], r["sigma_sigma"] = float(np.sqrt(sq_sel.mean())), float(np.sqrt(sq_sel).std())
        r["cell_index"] = off + c + 1
        r["ApprovedFits"] = _previous(v0, approved, off + c)[2]
        results.append({f: r[f] for f in RESULT_FIELDS})
        plots.append({"t_plot": t.copy(), "MS2_plot": m.copy(), "PP7_plot": p.copy(),
                      "simMS2": ms2[k, :n].copy(), "simPP7": pp7[k, :n].copy()})
        ch = {name + "_chain": th[:, THETA_INDEX[name]].copy() for name in _SCALARS}
        ch["dR_chain"] = th[:, 7:].copy()
        ch["s2chain"] = sq.copy()
        chains.append(ch)
        entries.append((demczs_entry if zs else demc_entry)(res, k, n, off + c + 1))
        if res.rank is not None:   # the rank diagnostics across the members, beside rhat_max / ess_min
            rk = rank_entry(res.rank, k, n, off + c + 1, n_pop)
            entries[-1].update({f: rk[f] for f in RANK_FIELDS if f not in DEMC_FIELDS})
    return FitResult(cl.name, results, plots, chains, res.accept_rate.mean(axis=1), int(res.n_evals.sum()),
                     res.kernel_ms, np.array(keep, np.int64) + off, res.pop[:, 0].copy(), MCMCsearch=searched,
                     **{"MCMCdemczs" if zs else "MCMCdemc": entries})


def _demczs_arg(arg):
    """``fit``'s ``demczs`` as keyword arguments of :func:`demczs`."""
    if not isinstance(arg, Mapping):
        raise ValueError(f"demczs must be a dict with keys among {DEMCZS_KEYS}")
    bad = sorted(set(arg) - set(DEMCZS_KEYS))
    if bad:
        raise ValueError(f"demczs has unknown keys {bad}: the keys are {DEMCZS_KEYS}")
    d = dict(arg)
    n_pop = d.setdefault("n_pop", 4)
    if isinstance(n_pop, bool) or int(n_pop) != n_pop or not 1 <= int(n_pop) <= 4096:
        raise ValueError("demczs n_pop must be an integer in [1, 4096]")
    n_gen = d.setdefault("n_gen", 1000)
    if isinstance(n_gen, bool) or int(n_gen) != n_gen or int(n_gen) < 1:
        raise ValueError("demczs n_gen must be an integer >= 1")
    m0 = d.get("m0")
    if m0 is not None and (isinstance(m0, bool) or int(m0) != m0 or int(m0) < max(3, int(n_pop))):
        raise ValueError("demczs m0 must be an integer >= max(3, n_pop): the chains start at the archive's first rows")
    if d.get("bounds", "reject") not in ("reject", "reflect"):
        raise ValueError("demczs bounds must be 'reject' or 'reflect'")
    if not isinstance(d.get("census", False), (bool, np.bool_)):
        raise ValueError("demczs census must be True or False")
    return d


def demczs_m0(cl: Cells, ids: Sequence[int]) -> int:
    """The default starting archive of :func:`demczs`: ``10 P`` rows, ``P = 7 + N`` of the longest of the cells ``ids``
    (ter Braak & Vrugt's ``M0 = 10 d``)."""
    return 10 * (7 + max((int(cl.lengths[int(c)]) for c in ids), default=0))


def demczs(lk, n_pop: int = 4, m0: Optional[int] = None, n_gen: int = 1000, thin: int = 1, n_burn: int = 0, seed: int = 0,
           cells: Optional[Sequence[int]] = None, v0=None, presearch=None, cell_offset: int = 0,
           ratePriorWidth: float = 50.0, jitter=None, CR: float = 0.2, gamma0: float = 0.0, jump_every: int = 10,
           updatesigma: bool = True, sigma2_0=1.0, append_every: int = 10, p_snooker: float = 0.1, rhat: bool = True,
           ess: bool = True, max_lag: int = 0, log_rows: int = 0, approved=None, rank=False, archive: bool = False,
           bounds: str = "reject", census: bool = False):
    """A DE-MC(zs) run (``Likelihood.demczs``; include/tci.h, ``tci_demczs_run``) of the cells ``cells`` (default: all)
    of ``lk``: ``n_pop`` chains per cell and a starting archive of ``m0`` rows (None: :func:`demczs_m0`, ``10 P`` of the
    longest selected cell; ``m0 >= max(3, n_pop)``). The archive ``z0`` is :func:`search_population` with ``m0`` members
    and the chains start at its first ``n_pop`` rows, so chain ``i`` starts at replicate ``i``'s x0. With ``presearch``
    (a dict for :func:`modesearch`, run here with ``m0`` members and the same ``seed``, or the ``(ModeSearch,
    SearchPlan)`` such a call returned) ``z0`` is the search's final population and the chains start at its best
    members (:func:`search_order`). Keys, seeds, ``jitter``, ``n_burn``, ``rank`` and the reductions are :func:`demc`'s;
    ``bounds`` and ``census`` are ``Likelihood.demczs``'s (``tci_demczs_run_bounds``).
    Returns ``(DemcZs, SearchPlan)``; row ``k`` of either is cell ``plan.cells[k]``, and ``plan.pop0`` is ``z0``."""
    cl: Cells = lk.cells
    ids = list(range(cl.n_cells)) if cells is None else [int(c) for c in cells]
    n_pop = int(n_pop)
    if isinstance(presearch, tuple):
        m0 = int(presearch[0].pop.shape[1]) if m0 is None else int(m0)
    m0 = demczs_m0(cl, kept_cells(cl, ids, v0, int(cell_offset))) if m0 is None else int(m0)
    if m0 < max(3, n_pop):
        raise ValueError("m0 must be >= max(3, n_pop): the chains start at the archive's first rows")
    if isinstance(presearch, tuple):
        sr, sp = presearch
        if sr.pop.shape[1] != m0:
            raise ValueError("the mode search's n_pop is not the sampler's m0")
    elif presearch is not None:
        if not isinstance(presearch, Mapping) or set(presearch) - {"n_gen", "F", "CR"}:
            raise ValueError("presearch must be a dict with keys among ('n_gen', 'F', 'CR') or a modesearch result")
        sr, sp = modesearch(lk, n_pop=m0, seed=seed, cells=ids, v0=v0, cell_offset=cell_offset,
                            ratePriorWidth=ratePriorWidth, approved=approved, **presearch)
    else:
        sr, sp = None, search_population(cl, ids, seed, m0, ratePriorWidth, v0, approved, cell_offset)
    if not sp.cells:
        return DemcZs.empty_zs(0, n_pop, sp.pop0.shape[2], int(n_gen), int(thin), 0, m0, max(int(append_every), 1), False), sp
    if sr is None:
        z0 = sp.pop0
        pop0 = z0[:, :n_pop]
    else:
        z0 = sr.pop
        pop0 = np.stack([z0[k, search_order(sr.f[k])[:n_pop]] for k in range(len(sp.cells))])
    jit = jitter
    if jit is None or np.ndim(jit) == 0:
        base = demc_jitter(cl, sp.cells, ratePriorWidth, v0, approved, cell_offset)
        jit = base if jit is None else float(jit) * base
    res = lk.demczs(pop0, z0, np.array(sp.cells, np.int32), sp.lower, sp.upper, sp.prior_mu, sp.prior_sig, jit,
                    sigma2_0=sigma2_0, n_gen=n_gen, thin=thin, jump_every=jump_every, CR=CR, gamma0=gamma0,
                    updatesigma=updatesigma, seed=int(seed) * 1000003 + 20201028,
                    keys=np.array(sp.cells, np.int64) + int(cell_offset), stats_from=n_burn, append_every=append_every,
                    p_snooker=p_snooker, rhat=rhat, ess=ess, max_lag=max_lag, log_rows=log_rows, rank=rank, archive=archive,
                    bounds=bounds, census=census)
    return res, sp


def demczs_entry(res: DemcZs, k: int, n: int, cell_index: int) -> Dict:
    """One ``MCMCdemczs`` entry (``DEMCZS_FIELDS``) from selected cell ``k`` of ``res``: :func:`demc_entry`'s values plus
    ``n_null`` per chain, ``snooker_rate`` (the share of snooker moves among the generations ``res`` logged, its first
    ``log_rows``: not of the whole run when the log is shorter; NaN without a log), ``m0`` and ``n_archive``. With the
    census: ``n_cross``, ``oob_lo`` and ``oob_hi`` ``[7 + n]`` summed over the cell's chains and ``oob_share`` ``[7 + n]``,
    ``(oob_lo + oob_hi)`` over the cell's bounds-rejected proposals. In reject mode that is the share of those proposals
    in which coordinate ``j`` had left; in reflect mode a leaving coordinate is reflected and the counters do not say
    which proposals were rejected, so it is NaN. With ``bounds='reflect'``: ``reflect_rate``, the evaluated proposals
    with at least one reflection over all proposals. None when the feature is off."""
    n_pop = int(res.pop.shape[1])
    snk = res.snooker[:, k * n_pop:(k + 1) * n_pop]
    d = dict(demc_entry(res, k, n, cell_index), n_null=res.n_null[k].copy(),
             snooker_rate=float(snk.mean()) if snk.size else float("nan"), m0=int(res.m0), n_archive=int(res.n_archive),
             n_cross=None, oob_lo=None, oob_hi=None, oob_share=None, reflect_rate=None)
    P = 7 + int(n)
    if res.census:
        for f in ("n_cross", "oob_lo", "oob_hi"):
            d[f] = getattr(res, f)[k, :, :P].astype(np.int64).sum(axis=0)
        rejected = int(res.n_oob[k].sum())
        left = (d["oob_lo"] + d["oob_hi"]).astype(np.float64)
        d["oob_share"] = left / rejected if res.bounds == "reject" and rejected else np.full(P, np.nan)
    if res.bounds == "reflect":
        d["reflect_rate"] = float(res.n_reflected[k].sum()) / (n_pop * res.n_gen) if res.n_gen else float("nan")
    return {f: d[f] for f in DEMCZS_FIELDS}


def search_order(f: np.ndarray) -> np.ndarray:
    """The members of one cell from best to worst: ascending ``f``, ties by index, NaN last."""
    f = np.asarray(f, np.float64)
    return np.lexsort((np.arange(len(f)), np.where(np.isnan(f), np.inf, f), np.isnan(f)))


def search_entry(sr: ModeSearch, k: int, n: int, cell_index: int) -> Dict:
    """One ``MCMCsearch`` entry (``SEARCH_FIELDS``) from selected cell ``k`` of ``sr``, a cell of ``n`` points."""
    n_pop = sr.pop.shape[1]
    d = dict(f_best=float(sr.f_best[k]), ss_best=float(sr.ss_best[k]), theta_best=sr.theta_best[k, :7 + n].copy(),
             f0_best=float(sr.f_trace[0, k]), f_trace=sr.f_trace[:, k].copy(), n_gen=int(sr.n_gen), n_pop=int(n_pop),
             n_evals=int(n_pop) * (int(sr.n_gen) + 1), cell_index=int(cell_index))
    return {f: d[f] for f in SEARCH_FIELDS}


def _temper_arg(temper):
    """(betas or None, rung count) of ``fit``'s ``temper``: None / 1 = no tempering; an integer rung count; or a
    sequence of inverse temperatures, strictly decreasing from 1 and positive."""
    if temper is None:
        return None, 1
    if isinstance(temper, bool):
        raise ValueError("temper must be a rung count or a sequence of inverse temperatures")
    if np.ndim(temper) == 0:
        if int(temper) != temper or int(temper) < 1:
            raise ValueError("temper must be an integer rung count >= 1 or a sequence of inverse temperatures")
        return None, int(temper)
    b = np.asarray(temper, np.float64).reshape(-1)
    if b.size < 1 or b[0] != 1.0 or not np.all(np.isfinite(b)) or np.any(b <= 0) or np.any(np.diff(b) >= 0):
        raise ValueError("temper as a sequence must start at 1 (the cold rung) and decrease strictly, every beta > 0")
    return b, int(b.size)


def temper_layout(lengths: Sequence[int], M: int, R: int, betas=None) -> Dict:
    """``beta`` and ``ladder`` of a tempered fit of ``K = len(lengths)`` cells of those point counts, ``M``
    replicates and ``R`` rungs, for :func:`dram_run`: chain ``(q * M + r) * K + k`` is rung ``q`` of ladder
    ``r * K + k`` (replicate ``r`` of cell ``k``). ``betas`` None: :func:`temper_ladder` of each cell's ``7 + N``."""
    K = len(lengths)
    beta = np.empty(M * R * K)
    ladder = np.empty(M * R * K, np.int32)
    for k, n in enumerate(lengths):
        b = temper_ladder(7 + int(n), R) if betas is None else np.asarray(betas, np.float64)
        for q in range(R):
            for r in range(M):
                beta[(q * M + r) * K + k] = b[q]
                ladder[(q * M + r) * K + k] = r * K + k
    return dict(beta=beta, ladder=ladder)


def temper_entry(res: DramResult, k: int, K: int, M: int, R: int, cell_index: int) -> Dict:
    """``MCMCtemper`` of fitted cell ``k`` from a tempered :func:`dram_run` in :func:`temper_layout`'s order."""
    t = res.temper
    idx = np.array([[(q * M + r) * K + k for q in range(R)] for r in range(M)])   # [M, R] chain of (replicate, rung)
    tried = t.swap_tried[idx[:, :-1]].astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        rate = np.where(tried > 0, t.swap_accepted[idx[:, :-1]] / tried, np.nan)
    d = dict(beta=t.beta[idx[0]].copy(), swap_rate=rate, swap_tried=tried, accept_rate=res.accept_rate[idx].copy(),
             swap_every=int(t.swap_every), n_events=int(t.n_events), n_chains=M * R, cell_index=int(cell_index))
    return {f: d[f] for f in TEMPER_FIELDS}


def stack_entries(lk, chain: np.ndarray, s2chain: np.ndarray, mean: np.ndarray, keep: Sequence[int], M: int,
                  nsample: int, cell_offset: int = 0, scratch_bytes: int = 0) -> List[Dict]:
    """``MCMCstack`` of a fit: ``chain`` ``[rows, M * K, ld]`` holds the post-burn-in kept rows of the ``M`` replicates
    of the ``K = len(keep)`` fitted cells (replicate-major, as :func:`fit` orders them), ``s2chain`` ``[>= rows, M * K]``
    every kept row's sigma2 (a row's sigma2 is among the last ``rows`` entries, as in :func:`fitcheck`) and ``mean``
    ``[M * K, ld]`` the chains' posterior means. :func:`predict_rows` of every chain go through ``Likelihood.loocheck``
    in one call, cell ``k``'s replicates as group ``k``."""
    K, rows = len(keep), chain.shape[0]
    idx = predict_rows(rows, nsample)
    if len(idx) < 32:
        raise ValueError(f"stack needs at least 32 kept post-burn-in rows and this fit kept {rows}")
    theta = np.ascontiguousarray(np.transpose(chain[idx], (1, 0, 2)))
    s2 = np.ascontiguousarray(np.asarray(s2chain, np.float64)[s2chain.shape[0] - rows:][idx].T)
    cid = np.tile(np.array(keep, np.int32), M)
    lc = lk.loocheck(theta, s2, cid, group=np.tile(np.arange(K, dtype=np.int32), M), scratch_bytes=scratch_bytes)
    out = []
    for k, c in enumerate(keep):
        n = int(lk.cells.lengths[c])
        w = lc.weight[k::K].copy()
        d = {f: getattr(lc, f)[k::K].copy() for f in ("elpd_loo", "p_loo", "khat_max", "n_khat_bad")}
        d.update(weights=w, elpd_loo_i=lc.elpd_loo_i[k, :, :n].copy(), khat_i=lc.khat_i[k, :, :n].copy(),
                 elpd_stack=float(lc.elpd_stack[k]), stacked_mean=w @ mean[k::K, :7 + n], n_samples=int(lc.n_samples),
                 cell_index=int(cell_offset) + c + 1)
        out.append({f: d[f] for f in STACK_FIELDS})
    return out


def lp_group_stats(lk, clp: ChainLp, K: int, M: int, max_lag: int = 0) -> Dict[str, np.ndarray]:
    """R-hat (classic, split), multi-chain ESS and MCSE of the ``lp`` trace across the ``M`` replicates of each of ``K``
    cells (chains replicate-major, as :func:`fit` orders them): the returned trace goes through
    ``Likelihood.chainrhat`` / ``chainess`` as a chain of one column, one group per cell. ``[K]`` each."""
    col = np.ascontiguousarray(clp.lp[:, :, None])
    group = np.tile(np.arange(K, dtype=np.int32), M)
    cr = lk.chainrhat(col, group=group)
    ce = lk.chainess(col, group=group, max_lag=max_lag)
    return {"lp_rhat": cr.rhat[:, 0].copy(), "lp_rhat_split": cr.rhat_split[:, 0].copy(), "lp_ess": ce.ess[:, 0].copy(),
            "lp_mcse": ce.mcse[:, 0].copy()}


def lp_entry(clp: ChainLp, k: int, n: int, cell_index: int, K: int = 1, M: int = 1, group: Optional[Dict] = None) -> Dict:
    """One ``MCMClp`` entry (``LP_FIELDS``) of a cell of ``n`` points from the chains ``k, k + K, ..`` (its ``M``
    replicates, replicate-major) of ``clp``. ``M == 1``: floats, ``best_row`` an int, ``best_dR`` ``[n]``, the traces
    ``[n_rows]``; ``M > 1``: a leading axis of ``M`` on each, and ``LP_GROUP_FIELDS`` from ``group``
    (:func:`lp_group_stats`, entry ``k``), ``ss_gap`` and ``best_replicate``."""
    rows = np.arange(M) * K + k
    d = {f: getattr(clp, f)[rows].copy() for f in LP_SCALARS + ("best_row",)}
    tb = clp.theta_best[rows]
    for name in _SCALARS:
        d["best_" + name] = tb[:, THETA_INDEX[name]].copy()
    d["best_dR"] = tb[:, 7:7 + n].copy()
    d["ss"], d["lp"] = clp.ss[:, rows].T.copy(), clp.lp[:, rows].T.copy()
    fields = LP_FIELDS
    if M == 1:
        d = {f: (int(v[0]) if f == "best_row" else float(v[0]) if v.ndim == 1 else v[0]) for f, v in d.items()}
    else:
        fields = LP_FIELDS + LP_GROUP_FIELDS
        for f in ("lp_rhat", "lp_rhat_split", "lp_ess", "lp_mcse"):
            d[f] = float(group[f][k])
        sm, lb = d["ss_mean"], d["lp_best"]
        d["ss_gap"] = float(np.max(sm) - np.min(sm))  # NaN when a replicate's is
        d["best_replicate"] = -1 if np.all(np.isnan(lb)) else int(np.nanargmax(lb))
    d["n_rows"] = int(clp.n_rows)
    d["n_chains"] = int(M)
    d["cell_index"] = int(cell_index)
    return {f: d[f] for f in fields}


def rank_entry(ck: ChainRank, k: int, n: int, cell_index: int, n_chains: int) -> Dict:
    """One ``MCMCrank`` entry (``RANK_FIELDS``) from group ``k`` of ``ck``, a cell of ``n`` points: the vectors trimmed
    to the cell's ``P = 7 + n`` theta columns with s2 appended as the last column, as :func:`ess_entry` lays columns out
    (``q`` ``[nq, P + 1]``, ``q_tail`` ``[2, P + 1]``). ``rhat_rank_max``, ``ess_bulk_min``, ``ess_tail_min``: the worst
    value over the ``P + 1`` columns, NaN left out (NaN when there is none)."""
    P = 7 + n
    d = {f: np.concatenate([getattr(ck, f)[k, :P], [getattr(ck, "s2_" + f)[k]]]) for f in RANK_VECTORS}
    for f in ("q", "q_tail"):
        d[f] = np.concatenate([getattr(ck, f)[k, :, :P], getattr(ck, "s2_" + f)[k][:, None]], axis=1)
    worst = lambda a, fn: float(fn(a[~np.isnan(a)])) if not np.all(np.isnan(a)) else float("nan")  # noqa: E731
    d["rhat_rank_max"] = worst(d["rhat_rank"], np.max)
    d["ess_bulk_min"], d["ess_tail_min"] = worst(d["ess_bulk"], np.min), worst(d["ess_tail"], np.min)
    d["probs"], d["tail"] = ck.probs.copy(), np.array(ck.tail, np.float64)
    d["max_lag"], d["n_rows"], d["n_chains"], d["cell_index"] = int(ck.max_lag), int(ck.n_rows), int(n_chains), int(cell_index)
    return {f: d[f] for f in RANK_FIELDS}


def ess_entry(ce: ChainEss, k: int, n: int, cell_index: int, n_chains: int) -> Dict:
    """One ``MCMCess`` entry (``ESS_FIELDS``) from group ``k`` of ``ce``, a cell of ``n`` points: the vectors trimmed
    to the cell's ``P = 7 + n`` theta columns with s2 appended as the last column, as :func:`rhat_entry` lays columns
    out. ``ess_min``: the smallest classic or split ess over the ``P + 1`` columns, NaN left out (NaN when there is
    none)."""
    P = 7 + n
    d = {f: np.concatenate([getattr(ce, f)[k, :P], [getattr(ce, "s2_" + f)[k]]])
         for f in ("ess", "ess_split", "tau", "tau_split", "mcse", "window", "window_split")}
    both = np.concatenate([d["ess"], d["ess_split"]])
    d["ess_min"] = float(np.min(both[~np.isnan(both)])) if not np.all(np.isnan(both)) else float("nan")
    d["max_lag"] = int(ce.max_lag)
    d["n_rows"] = int(ce.n_rows)
    d["n_chains"] = int(n_chains)
    d["cell_index"] = int(cell_index)
    return {f: d[f] for f in ESS_FIELDS}


def rhat_entry(cr: ChainRhat, k: int, n: int, cell_index: int, mean_rep: np.ndarray, accept_rep: np.ndarray) -> Dict:
    """One ``MCMCrhat`` entry (``RHAT_FIELDS``) from group ``k`` of ``cr``, a cell of ``n`` points: the four vectors
    trimmed to the cell's ``P = 7 + n`` theta columns (order: ``THETA_INDEX``, then dR) with s2 appended as the last
    column, as :func:`dens_entry` lays columns out. ``mean_rep`` ``[M, >= P]`` and ``accept_rep`` ``[M]``: the
    replicates' posterior means and acceptance rates. ``rhat_max``: the largest classic or split factor over the
    ``P + 1`` columns, NaN left out (NaN when there is none)."""
    P = 7 + n
    join = lambda a, b: np.concatenate([a[k, :P], [b[k]]])  # noqa: E731
    d = {"rhat": join(cr.rhat, cr.s2_rhat), "rhat_split": join(cr.rhat_split, cr.s2_rhat_split),
         "pooled_mean": join(cr.pooled_mean, cr.s2_pooled_mean), "pooled_std": join(cr.pooled_std, cr.s2_pooled_std),
         "mean_rep": np.array(mean_rep[:, :P]), "accept_rep": np.array(accept_rep)}
    both = np.concatenate([d["rhat"], d["rhat_split"]])
    d["rhat_max"] = float(np.max(both[~np.isnan(both)])) if not np.all(np.isnan(both)) else float("nan")
    d["n_rows"] = int(cr.n_rows)
    d["n_chains"] = int(len(d["accept_rep"]))
    d["cell_index"] = int(cell_index)
    return {f: d[f] for f in RHAT_FIELDS}


def dens_entry(cd: ChainDens, k: int, n: int, cell_index: int) -> Dict:
    """One ``MCMCdens`` entry (``DENS_FIELDS``) from chain ``k`` of ``cd``, a cell of ``n`` points: the arrays
    trimmed to the cell's ``P = 7 + n`` theta columns (order: ``THETA_INDEX``, then dR) with s2 appended as the
    last column: ``grid`` and ``dens`` ``[G, P + 1]``, ``counts`` ``[B, P + 1]``, ``range`` ``[2, P + 1]``, ``bw`` ``[P + 1]``."""
    P = 7 + n
    join = lambda a, b: np.concatenate([a[k][..., :P], np.asarray(b[k])[..., None]], axis=-1)  # noqa: E731
    return {"grid": join(cd.grid(), cd.s2_grid()), "dens": join(cd.dens, cd.s2_dens),
            "counts": join(cd.counts, cd.s2_counts), "range": join(cd.range, cd.s2_range),
            "bw": join(cd.bw, cd.s2_bw), "n_rows": int(cd.n_rows), "cell_index": int(cell_index)}


def cov_entry(cc: ChainCov, k: int, n: int, cell_index: int) -> Dict:
    """One ``MCMCcov`` entry (``COV_FIELDS``) from chain ``k`` of ``cc``, a cell of ``n`` points: the
    matrices trimmed to the cell's ``P = 7 + n`` columns (theta order: ``THETA_INDEX``, then dR)."""
    P = 7 + n
    return {"mean": cc.mean[k, :P].copy(), "cov": cc.cov[k, :P, :P].copy(), "corr": cc.corr[k, :P, :P].copy(),
            "n_rows": int(cc.n_rows), "cell_index": int(cell_index)}


def quant_entry(cq: ChainQuant, k: int, n: int, cell_index: int) -> Dict:
    """One ``MCMCquant`` entry (``QUANT_FIELDS``) from chain ``k`` of ``cq``, a cell of ``n`` points: ``[nq]`` per
    scalar parameter and for s2, ``[nq, n]`` for dR, at ``probs``."""
    d = {"q_" + name: cq.q[k, :, THETA_INDEX[name]].copy() for name in _SCALARS}
    d["q_dR"] = cq.q[k, :, 7:7 + n].copy()
    d["q_s2"] = cq.s2_q[k].copy()
    d["probs"] = cq.probs.copy()
    d["n_rows"] = int(cq.n_rows)
    d["cell_index"] = int(cell_index)
    return {f: d[f] for f in QUANT_FIELDS}


def diag_entry(st: ChainStats, k: int, n: int, cell_index: int) -> Dict:
    """One ``MCMCdiag`` entry (``DIAG_FIELDS``) from chain ``k`` of ``st``, a cell of ``n`` points.
    ``ess_min = n_rows / max tau`` over the cell's parameters (s2 left out): the effective sample
    size of its slowest parameter; NaN when that tau is NaN, 0 when it is +Inf."""
    d = {}
    for stat, arr, s2 in (("mcerr", st.mcerr, st.s2_mcerr), ("tau", st.tau, st.s2_tau),
                          ("geweke_p", st.geweke_p, st.s2_geweke_p)):
        for name in _SCALARS:
            d[f"{stat}_{name}"] = float(arr[k, THETA_INDEX[name]])
        d[f"{stat}_dR"] = arr[k, 7:7 + n].copy()
        d[f"{stat}_s2"] = float(s2[k])
    tau = st.tau[k, :7 + n]
    d["n_rows"] = int(st.n_rows)
    with np.errstate(divide="ignore", invalid="ignore"):
        d["ess_min"] = float(np.float64(st.n_rows) / np.max(tau)) if tau.size else float("nan")
    d["cell_index"] = int(cell_index)
    return {f: d[f] for f in DIAG_FIELDS}


# ---------------------------------------------------------------------------
# Posterior predictive envelopes (mcmcstat's mcmcpred on the fit's chain)
# ---------------------------------------------------------------------------


def predict_rows(rows: int, nsample: int) -> np.ndarray:
    """Indices of the chain rows :func:`predict` simulates: all of them when there are fewer than
    ``nsample``, else ``round(linspace(0, rows-1, nsample))``."""
    rows, nsample = int(rows), int(nsample)
    if nsample < 1:
        raise ValueError("nsample must be >= 1")
    if rows < nsample:
        return np.arange(rows, dtype=np.int64)
    return np.round(np.linspace(0, rows - 1, nsample)).astype(np.int64)


def chain_theta(chain: Mapping, n: int, idx: np.ndarray) -> np.ndarray:
    """Rows ``idx`` of one ``MCMCchain`` entry as theta rows in the ABI order
    ``[v, tau, ton, MS2_basal, PP7_basal, A, R, dR_1 .. dR_n]`` (include/tci.h)."""
    th = np.zeros((len(idx), 7 + n))
    for name, col in THETA_INDEX.items():
        th[:, col] = np.asarray(chain[name + "_chain"], np.float64).reshape(-1)[idx]
    th[:, 7:] = np.asarray(chain["dR_chain"], np.float64).reshape(-1, n)[idx]
    return th


def predict(lk, fit_result: FitResult, nsample: int = 500, probs=(0.025, 0.5, 0.975), grid: str = "raw",
            cell_offset: int = 0, scratch_bytes: int = 0) -> FitResult:
    """Predictive bands of every fitted cell, as mcmcstat's ``mcmcpred`` + ``mcmcpredplot`` give
    them: the forward model at ``nsample`` posterior samples of the cell's chain and, at every
    acquisition time, the ``probs`` quantiles of the simulated MS2 and PP7 signals (``plims``), all on
    the device (``Likelihood.predict``). Adds ``predMS2`` and ``predPP7`` (nq x N) and ``pred_probs`` to
    each ``MCMCplot`` entry of ``fit_result`` and returns it.

    The samples are the post-burn-in rows kept in ``MCMCchain`` (fit with ``thin > 0``). mcmcpred
    draws ``nsample`` chain rows at random; here the choice is deterministic: every row when a cell
    has fewer than ``nsample``, else rows ``round(linspace(0, rows-1, nsample))``, so a prediction
    can be reproduced from the result file alone. ``nsample`` is at most 4096. Observation-noise bands
    (mcmcpred's ``obslims``) are not computed. ``cell_offset``: as in :func:`fit`."""
    if not fit_result.MCMCchain or any(not c or np.size(c.get("v_chain", ())) == 0 for c in fit_result.MCMCchain):
        raise ValueError("predict needs the fit's chain rows and this fit kept none: run fit(..., thin=k) with "
                         "k > 0 and n_burn <= n_steps")
    pr = np.ascontiguousarray(np.atleast_1d(probs), np.float64)
    cl: Cells = lk.cells
    groups: Dict[int, List[int]] = {}
    thetas = []
    for k, ch in enumerate(fit_result.MCMCchain):
        c = int(fit_result.cell_index[k]) - int(cell_offset)
        n = int(cl.lengths[c])
        th = chain_theta(ch, n, predict_rows(np.size(ch["v_chain"]), nsample))
        thetas.append(th)
        groups.setdefault(len(th), []).append(k)
    for S, ks in groups.items():   # one device call per distinct sample count (a fit has one)
        ld = max(thetas[k].shape[1] for k in ks)
        theta = np.zeros((len(ks), S, ld))
        for i, k in enumerate(ks):
            theta[i, :, :thetas[k].shape[1]] = thetas[k]
        cid = np.array([int(fit_result.cell_index[k]) - int(cell_offset) for k in ks], np.int32)
        ms2_q, pp7_q = lk.predict(theta, cid, probs=pr, grid=grid, scratch_bytes=scratch_bytes)
        for i, k in enumerate(ks):
            n = thetas[k].shape[1] - 7
            fit_result.MCMCplot[k].update(predMS2=ms2_q[i, :, :n].copy(), predPP7=pp7_q[i, :, :n].copy(),
                                          pred_probs=pr.copy())
    return fit_result


# ---------------------------------------------------------------------------
# Posterior predictive fit checks (WAIC, PIT, coverage, reduced chi^2, Durbin-Watson)
# ---------------------------------------------------------------------------


def check_entry(fc: FitCheck, k: int, n: int, cell_index: int) -> Dict:
    """One ``MCMCcheck`` entry (``CHECK_FIELDS``) from selected cell ``k`` of ``fc``, a cell of ``n`` points: the
    pointwise vectors trimmed to ``[2, n]``, the per-cell scalars, ``waic = -2 elpd_waic``."""
    d = {f: getattr(fc, f)[k, :, :n].copy() for f in FITCHECK_POINTWISE}
    d["n_obs"] = int(fc.n_obs[k])
    for f in ("lppd", "p_waic", "elpd_waic", "chi2"):
        d[f] = float(getattr(fc, f)[k])
    d["waic"] = -2.0 * d["elpd_waic"]
    d["coverage"] = fc.coverage[k].copy()
    d["dw"] = fc.dw[k].copy()
    d["levels"] = fc.levels.copy()
    d["n_samples"] = int(fc.n_samples)
    d["cell_index"] = int(cell_index)
    return {f: d[f] for f in CHECK_FIELDS}


def fitcheck(lk, fit_result: FitResult, nsample: int = 500, levels=(0.5, 0.95), cell_offset: int = 0,
             scratch_bytes: int = 0) -> FitResult:
    """Posterior predictive fit checks of every fitted cell on the device (``Likelihood.fitcheck``; formulas in
    ``include/tci.h``): each datum is scored under the Gaussian mixture that ``nsample`` posterior samples
    (theta, sigma2) of the cell's chain define. Sets ``fit_result.MCMCcheck`` (``CHECK_FIELDS`` per fitted cell) and
    returns ``fit_result``.

    The samples are the rows :func:`predict` takes (:func:`predict_rows` of the post-burn-in rows kept in
    ``MCMCchain``; fit with ``thin > 0``). ``s2chain`` is stored unsliced by ``n_burn``, so a row's sigma2 is read
    from the last ``len(v_chain)`` entries of the cell's ``s2chain``: the entries of the same kept rows.
    ``nsample`` is at most 4096. ``cell_offset``: as in :func:`fit`."""
    if not fit_result.MCMCchain or any(not c or np.size(c.get("v_chain", ())) == 0 for c in fit_result.MCMCchain):
        raise ValueError("fitcheck needs the fit's chain rows and this fit kept none: run fit(..., thin=k) with "
                         "k > 0 and n_burn <= n_steps")
    cl: Cells = lk.cells
    groups: Dict[int, List[int]] = {}
    thetas, s2s = [], []
    for k, ch in enumerate(fit_result.MCMCchain):
        c = int(fit_result.cell_index[k]) - int(cell_offset)
        n = int(cl.lengths[c])
        rows = int(np.size(ch["v_chain"]))
        s2c = np.asarray(ch["s2chain"], np.float64).reshape(-1)
        if len(s2c) < rows:
            raise ValueError(f"fitted cell {k}: s2chain has {len(s2c)} entries for {rows} chain rows")
        idx = predict_rows(rows, nsample)
        thetas.append(chain_theta(ch, n, idx))
        s2s.append(s2c[len(s2c) - rows:][idx])
        groups.setdefault(len(idx), []).append(k)
    entries: List[Optional[Dict]] = [None] * len(thetas)
    for S, ks in groups.items():   # one device call per distinct sample count (a fit has one)
        ld = max(thetas[k].shape[1] for k in ks)
        theta = np.zeros((len(ks), S, ld))
        for i, k in enumerate(ks):
            theta[i, :, :thetas[k].shape[1]] = thetas[k]
        cid = np.array([int(fit_result.cell_index[k]) - int(cell_offset) for k in ks], np.int32)
        fc = lk.fitcheck(theta, np.stack([s2s[k] for k in ks]), cid, levels=levels, scratch_bytes=scratch_bytes)
        for i, k in enumerate(ks):
            entries[k] = check_entry(fc, i, thetas[k].shape[1] - 7, int(fit_result.cell_index[k]) + 1)
    fit_result.MCMCcheck = entries
    return fit_result


# ---------------------------------------------------------------------------
# Result files (TranscriptionCycleMCMC.m:371-378)
# ---------------------------------------------------------------------------


def _struct_array(items: List[Dict], fields: Sequence[str]) -> np.ndarray:
    arr = np.empty((1, len(items)), dtype=[(f, object) for f in fields])
    for i, it in enumerate(items):
        for f in fields:
            v = it.get(f, np.zeros((0, 0)))
            if isinstance(v, np.ndarray) and v.ndim == 1:
                v = v[None, :]  # MATLAB row vectors
            arr[0, i][f] = v
    return arr


def save_results(fit_result: FitResult, save_loc: str = ".", date: Optional[str] = None):
    """Write ``<date>-<DatasetName>.mat`` (MCMCresults, MCMCplot, DatasetName) and
    ``<date>-<DatasetName>_RawChain.mat`` (MCMCchain), as the reference does (:373-378).
    ``date`` defaults to MATLAB's ``date`` format (dd-Mmm-yyyy). Returns the two paths."""
    import scipy.io as sio

    date = date or datetime.date.today().strftime("%d-%b-%Y")
    base = os.path.join(save_loc, f"{date}-{fit_result.DatasetName}")
    # the predictive bands only after predict(): a fit without them writes the same file as before
    plot_fields = PLOT_FIELDS + (PRED_FIELDS if any("predMS2" in p for p in fit_result.MCMCplot) else ())
    variables = {"MCMCresults": _struct_array(fit_result.MCMCresults, RESULT_FIELDS),
                 "MCMCplot": _struct_array(fit_result.MCMCplot, plot_fields),
                 "DatasetName": fit_result.DatasetName}
    if fit_result.MCMCdiag is not None:  # only a fit with diagnostics: any other writes the same file as before
        variables["MCMCdiag"] = _struct_array(fit_result.MCMCdiag, DIAG_FIELDS)
    if fit_result.MCMCcov is not None:  # only a fit with covariance=True
        variables["MCMCcov"] = _struct_array(fit_result.MCMCcov, COV_FIELDS)
    if fit_result.MCMCquant is not None:  # only a fit with quantiles=probs
        variables["MCMCquant"] = _struct_array(fit_result.MCMCquant, QUANT_FIELDS)
    if fit_result.MCMCrhat is not None:  # only a fit with replicates > 1 or rhat=True
        variables["MCMCrhat"] = _struct_array(fit_result.MCMCrhat, RHAT_FIELDS)
    if fit_result.MCMCess is not None:  # only a fit with ess=True
        variables["MCMCess"] = _struct_array(fit_result.MCMCess, ESS_FIELDS)
    if fit_result.MCMCrank is not None:  # only a fit with rank=True
        variables["MCMCrank"] = _struct_array(fit_result.MCMCrank, RANK_FIELDS)
    if fit_result.MCMCdens is not None:  # only a fit with density=True
        variables["MCMCdens"] = _struct_array(fit_result.MCMCdens, DENS_FIELDS)
    if fit_result.MCMClp is not None:  # only a fit with logpost=True
        lp_fields = LP_FIELDS + (LP_GROUP_FIELDS if any("lp_rhat" in e for e in fit_result.MCMClp) else ())
        variables["MCMClp"] = _struct_array(fit_result.MCMClp, lp_fields)
    if fit_result.MCMCstack is not None:  # only a fit with stack=nsample
        variables["MCMCstack"] = _struct_array(fit_result.MCMCstack, STACK_FIELDS)
    if fit_result.MCMCcheck is not None:  # only after fitcheck()
        variables["MCMCcheck"] = _struct_array(fit_result.MCMCcheck, CHECK_FIELDS)
    if fit_result.MCMCsearch is not None:  # only a fit with presearch
        variables["MCMCsearch"] = _struct_array(fit_result.MCMCsearch, SEARCH_FIELDS)
    sio.savemat(base + ".mat", variables)
    chains = [c if c else {f: np.zeros((0, 1)) for f in CHAIN_FIELDS} for c in fit_result.MCMCchain]
    for c in chains:  # chains are column vectors in the reference (chain(n_burn:end, k))
        for f in CHAIN_FIELDS:
            if f in c and isinstance(c[f], np.ndarray) and c[f].ndim == 1:
                c[f] = c[f][:, None]
    sio.savemat(base + "_RawChain.mat", {"MCMCchain": _struct_array(chains, CHAIN_FIELDS)})
    return base + ".mat", base + "_RawChain.mat"


def load_previous(results_path: str) -> Dict[int, PreviousFit]:
    """``loadPrevious`` (hierarchical fit, TranscriptionCycleMCMC.m:84-107): the ``MCMCresults``
    of an earlier result file as ``cell_index -> PreviousFit(mean_v, ApprovedFits)``. The fit
    looks each cell up by ``cell_index`` (:194), so cells missing from the file (pruned there,
    :359-369) are skipped, never shifted. A repeated cell_index keeps its first entry (MATLAB's
    ``v0 = MCMCresults(cellToload).mean_v`` takes the first of a comma list). Read with
    scipy.io.loadmat: a data reader, nothing executes."""
    import scipy.io as sio

    d = sio.loadmat(results_path, squeeze_me=True, struct_as_record=False)
    out: Dict[int, PreviousFit] = {}
    for r in np.atleast_1d(d["MCMCresults"]):
        ci = getattr(r, "cell_index", None)
        if ci is None or np.size(ci) != 1:
            continue
        v = getattr(r, "mean_v", None)
        v = float(v) if v is not None and np.size(v) == 1 else None   # [] -> skipped at :196
        a = getattr(r, "ApprovedFits", 0)
        a = int(a) if np.size(a) == 1 else 0
        out.setdefault(int(ci), PreviousFit(v, a))
    return out


def load_previous_v(results_path: str) -> Dict[int, float]:
    """``cell_index -> mean_v`` of an earlier result file (entries with a usable rate only)."""
    return {c: p.mean_v for c, p in load_previous(results_path).items()
            if p.mean_v is not None and math.isfinite(p.mean_v)}
