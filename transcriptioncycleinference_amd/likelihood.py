"""Batched likelihood on one MI355X: a resident cell table + the HIP kernels behind ``include/tci.h``.

``Likelihood`` is the batched form of mcmcstat's ``model.ssfun`` (set at
``TranscriptionCycleMCMC.m:186,258``; contract ``ss = ssfun(theta, data)``): the parfor over cells
(``:161``) becomes one launch over B = cells x proposals rows.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from typing import Optional, Sequence

import numpy as np

from . import _lib
from .construct import Construct, as_construct
from .data import Cells


@dataclasses.dataclass
class ChainStats:
    """Per-column chain diagnostics (``tci_chainstats_outputs``): arrays ``[n_chains, ld]`` for the
    parameters and ``[n_chains]`` for s2."""

    mcerr: np.ndarray
    tau: np.ndarray
    tau_window: np.ndarray
    geweke_z: np.ndarray
    geweke_p: np.ndarray
    s2_mcerr: np.ndarray
    s2_tau: np.ndarray
    s2_tau_window: np.ndarray
    s2_geweke_z: np.ndarray
    s2_geweke_p: np.ndarray
    n_rows: int = 0
    kernel_ms: float = 0.0

    @classmethod
    def empty(cls, n: int, ld: int) -> "ChainStats":
        d = lambda *s: np.full(s, np.nan)  # noqa: E731
        w = lambda *s: np.full(s, -1, np.int32)  # noqa: E731
        return cls(d(n, ld), d(n, ld), w(n, ld), d(n, ld), d(n, ld), d(n), d(n), w(n), d(n), d(n))

    def to_c(self) -> "_lib.tci_chainstats_outputs":
        P, W = (lambda a: _lib.ptr(a, _lib._dp)), (lambda a: _lib.ptr(a, _lib._i32p))  # noqa: E731
        return _lib.tci_chainstats_outputs(P(self.mcerr), P(self.tau), P(self.geweke_z), P(self.geweke_p),
                                           W(self.tau_window), P(self.s2_mcerr), P(self.s2_tau), P(self.s2_geweke_z),
                                           P(self.s2_geweke_p), W(self.s2_tau_window), 0, 0.0)


@dataclasses.dataclass
class ChainCov:
    """Per-chain posterior moments (``tci_chaincov_outputs``): ``mean`` ``[n_chains, ld]``, ``cov`` and
    ``corr`` ``[n_chains, ld, ld]``; padding is NaN."""

    mean: np.ndarray
    cov: np.ndarray
    corr: np.ndarray
    n_rows: int = 0
    kernel_ms: float = 0.0

    @classmethod
    def empty(cls, n: int, ld: int) -> "ChainCov":
        return cls(np.full((n, ld), np.nan), np.full((n, ld, ld), np.nan), np.full((n, ld, ld), np.nan))

    def to_c(self) -> "_lib.tci_chaincov_outputs":
        P = lambda a: _lib.ptr(a, _lib._dp)  # noqa: E731
        return _lib.tci_chaincov_outputs(P(self.mean), P(self.cov), P(self.corr), 0, 0.0)


def quant_probs(probs) -> np.ndarray:
    """``probs`` as the float64 vector ``tci_chainquant_options`` takes: 1 to 16 values in [0, 1]."""
    pr = np.ascontiguousarray(np.atleast_1d(np.asarray(probs, np.float64)))
    if pr.ndim != 1 or not 1 <= len(pr) <= 16:
        raise ValueError("probs must hold 1 to 16 probabilities")
    if not np.all((pr >= 0) & (pr <= 1)):
        raise ValueError("probs must be finite and in [0, 1]")
    return pr


@dataclasses.dataclass
class ChainQuant:
    """Per-column posterior quantiles (``tci_chainquant_outputs``): ``q`` ``[n_chains, nq, ld]`` and ``s2_q``
    ``[n_chains, nq]`` at the probabilities ``probs`` ``[nq]``; padding is NaN."""

    q: np.ndarray
    s2_q: np.ndarray
    probs: np.ndarray
    n_rows: int = 0
    kernel_ms: float = 0.0

    @classmethod
    def empty(cls, n: int, ld: int, probs=(0.025, 0.5, 0.975)) -> "ChainQuant":
        pr = quant_probs(probs)
        return cls(np.full((n, len(pr), ld), np.nan), np.full((n, len(pr)), np.nan), pr)

    def options(self) -> "_lib.tci_chainquant_options":
        o = _lib.tci_chainquant_options(len(self.probs))
        o.probs[:len(self.probs)] = self.probs.tolist()
        return o

    def to_c(self) -> "_lib.tci_chainquant_outputs":
        P = lambda a: _lib.ptr(a, _lib._dp)  # noqa: E731
        return _lib.tci_chainquant_outputs(P(self.q), P(self.s2_q), 0, 0.0)


def dens_options(n_grid=100, n_bins=20, bw_scale=1.0):
    """The three options of ``tci_chaindens_options``, checked: ``n_grid`` in 2..256, ``n_bins`` in 1..256,
    ``bw_scale`` finite and > 0."""
    G, B, s = int(n_grid), int(n_bins), float(bw_scale)
    if G != n_grid or not 2 <= G <= 256:
        raise ValueError("n_grid must be an integer in [2, 256]")
    if B != n_bins or not 1 <= B <= 256:
        raise ValueError("n_bins must be an integer in [1, 256]")
    if not (np.isfinite(s) and s > 0):
        raise ValueError("bw_scale must be finite and > 0")
    return G, B, s


def dens_grid(lo_hi: np.ndarray, n_grid: int) -> np.ndarray:
    """The density grid of ``include/tci.h`` from ``range``: ``lo_hi`` is ``[..., 2, m]`` (xmin, xmax), the result
    ``[..., n_grid, m]``; ``lo = xmin - 0.08 r``, ``hi = xmax + 0.08 r``, ``step = (hi - lo) / (G - 1)``,
    ``g_k = lo + k step``, every operation rounded once (numpy fuses nothing): the bits the device used."""
    lo_hi = np.asarray(lo_hi, np.float64)
    xmin, xmax = lo_hi[..., 0:1, :], lo_hi[..., 1:2, :]
    with np.errstate(invalid="ignore", over="ignore"):
        r = xmax - xmin
        w = 0.08 * r
        lo, hi = xmin - w, xmax + w
        step = (hi - lo) / np.float64(n_grid - 1)
        k = np.arange(n_grid, dtype=np.float64).reshape((n_grid, 1))
        return lo + k * step


@dataclasses.dataclass
class ChainDens:
    """Per-column marginal densities and histograms (``tci_chaindens_outputs``): ``range`` ``[n_chains, 2, ld]``
    (xmin, xmax), ``bw`` ``[n_chains, ld]``, ``dens`` ``[n_chains, n_grid, ld]`` on :meth:`grid`, ``counts``
    ``[n_chains, n_bins, ld]`` (int32) over ``n_bins`` equal bins of ``range``, and the same for s2 without the
    last axis; padding is NaN (counts -1)."""

    range: np.ndarray
    bw: np.ndarray
    dens: np.ndarray
    counts: np.ndarray
    s2_range: np.ndarray
    s2_bw: np.ndarray
    s2_dens: np.ndarray
    s2_counts: np.ndarray
    n_grid: int = 100
    n_bins: int = 20
    bw_scale: float = 1.0
    n_rows: int = 0
    kernel_ms: float = 0.0

    @classmethod
    def empty(cls, n: int, ld: int, n_grid=100, n_bins=20, bw_scale=1.0) -> "ChainDens":
        G, B, s = dens_options(n_grid, n_bins, bw_scale)
        d = lambda *sh: np.full(sh, np.nan)  # noqa: E731
        w = lambda *sh: np.full(sh, -1, np.int32)  # noqa: E731
        return cls(d(n, 2, ld), d(n, ld), d(n, G, ld), w(n, B, ld), d(n, 2), d(n), d(n, G), w(n, B), G, B, s)

    def options(self) -> "_lib.tci_chaindens_options":
        return _lib.tci_chaindens_options(int(self.n_grid), int(self.n_bins), float(self.bw_scale))

    def to_c(self) -> "_lib.tci_chaindens_outputs":
        P, W = (lambda a: _lib.ptr(a, _lib._dp)), (lambda a: _lib.ptr(a, _lib._i32p))  # noqa: E731
        return _lib.tci_chaindens_outputs(P(self.range), P(self.bw), P(self.dens), W(self.counts), P(self.s2_range),
                                          P(self.s2_bw), P(self.s2_dens), W(self.s2_counts), 0, 0.0)

    def grid(self) -> np.ndarray:
        """``[n_chains, n_grid, ld]``: the points ``dens`` is given at (:func:`dens_grid` of ``range``)."""
        return dens_grid(self.range, self.n_grid)

    def s2_grid(self) -> np.ndarray:
        """``[n_chains, n_grid]``: the points of ``s2_dens``."""
        return dens_grid(self.s2_range.T[None], self.n_grid)[0].T.copy()


def rhat_groups(group, n: int, npar=None):
    """``group`` as the int32 vector ``tci_chainrhat`` takes and the number of groups: None = all ``n`` chains in
    group 0; else one id per chain, -1 = no group, and ``n_groups = max id + 1`` (at least 1). ``npar`` (one per
    chain, when given): the chains of a group must have one."""
    if group is None:
        g = np.zeros(n, np.int32)
    else:
        g = np.asarray(group)
        if g.shape != (n,) or not np.issubdtype(g.dtype, np.integer):
            raise ValueError("group must hold one integer id per chain")
        if g.min() < -1 or g.max() >= n:
            raise ValueError("group ids must be in [-1, n_chains)")
        g = np.ascontiguousarray(g, np.int32)
    if npar is not None:
        for k in np.unique(g[g >= 0]):
            if len(np.unique(np.asarray(npar)[g == k])) > 1:
                raise ValueError(f"group {int(k)} has chains of different npar")
    return g, max(int(g.max()) + 1, 1)


@dataclasses.dataclass
class ChainRhat:
    """Per-group convergence across replicate chains (``tci_chainrhat_outputs``): the classic and the split
    potential scale reduction factor and the pooled posterior mean and standard deviation, ``[n_groups, ld]`` for the
    parameters and ``[n_groups]`` for s2; padding is NaN."""

    rhat: np.ndarray
    rhat_split: np.ndarray
    pooled_mean: np.ndarray
    pooled_std: np.ndarray
    s2_rhat: np.ndarray
    s2_rhat_split: np.ndarray
    s2_pooled_mean: np.ndarray
    s2_pooled_std: np.ndarray
    n_rows: int = 0
    kernel_ms: float = 0.0

    @classmethod
    def empty(cls, n_groups: int, ld: int) -> "ChainRhat":
        d = lambda *s: np.full(s, np.nan)  # noqa: E731
        g = int(n_groups)
        return cls(d(g, ld), d(g, ld), d(g, ld), d(g, ld), d(g), d(g), d(g), d(g))

    def options(self) -> "_lib.tci_chainrhat_options":
        return _lib.tci_chainrhat_options(0)

    def to_c(self) -> "_lib.tci_chainrhat_outputs":
        P = lambda a: _lib.ptr(a, _lib._dp)  # noqa: E731
        return _lib.tci_chainrhat_outputs(P(self.rhat), P(self.rhat_split), P(self.pooled_mean), P(self.pooled_std),
                                          P(self.s2_rhat), P(self.s2_rhat_split), P(self.s2_pooled_mean),
                                          P(self.s2_pooled_std), 0, 0.0)


ESS_OUTPUTS = ("ess", "ess_split", "tau", "tau_split", "mcse")
ESS_WINDOWS = ("window", "window_split")


@dataclasses.dataclass
class ChainEss:
    """Per-group effective sample size across replicate chains (``tci_chainess_outputs``): the multi-chain ESS and
    autocorrelation time, classic and split, the pooled mean's Monte-Carlo standard error and the lags summed,
    ``[n_groups, ld]`` for the parameters and ``[n_groups]`` for s2; padding is NaN / -1."""

    ess: np.ndarray
    ess_split: np.ndarray
    tau: np.ndarray
    tau_split: np.ndarray
    mcse: np.ndarray
    window: np.ndarray
    window_split: np.ndarray
    s2_ess: np.ndarray
    s2_ess_split: np.ndarray
    s2_tau: np.ndarray
    s2_tau_split: np.ndarray
    s2_mcse: np.ndarray
    s2_window: np.ndarray
    s2_window_split: np.ndarray
    max_lag: int = 0
    n_rows: int = 0
    kernel_ms: float = 0.0

    @classmethod
    def empty(cls, n_groups: int, ld: int, max_lag: int = 0) -> "ChainEss":
        d = lambda *s: np.full(s, np.nan)  # noqa: E731
        w = lambda *s: np.full(s, -1, np.int32)  # noqa: E731
        g = int(n_groups)
        if int(max_lag) != max_lag or int(max_lag) < 0:
            raise ValueError("max_lag must be an integer >= 0")
        return cls(d(g, ld), d(g, ld), d(g, ld), d(g, ld), d(g, ld), w(g, ld), w(g, ld), d(g), d(g), d(g), d(g), d(g),
                   w(g), w(g), int(max_lag))

    def options(self) -> "_lib.tci_chainess_options":
        return _lib.tci_chainess_options(self.max_lag, 0)

    def to_c(self) -> "_lib.tci_chainess_outputs":
        P = lambda a: _lib.ptr(a, _lib._dp)  # noqa: E731
        I = lambda a: _lib.ptr(a, _lib._i32p)  # noqa: E731,E741
        return _lib.tci_chainess_outputs(P(self.ess), P(self.ess_split), P(self.tau), P(self.tau_split), P(self.mcse),
                                         I(self.window), I(self.window_split), P(self.s2_ess), P(self.s2_ess_split),
                                         P(self.s2_tau), P(self.s2_tau_split), P(self.s2_mcse), I(self.s2_window),
                                         I(self.s2_window_split), 0, 0.0)


@dataclasses.dataclass
class ChainRank:
    """Per-group rank diagnostics across replicate chains (``tci_chainrank_outputs``; Vehtari et al. 2021): the pooled
    quantiles ``q`` ``[n_groups, nq, ld]`` and ``q_tail`` ``[n_groups, 2, ld]``, the rank-normalised split R-hat
    (``rhat_bulk``, ``rhat_folded`` and their maximum ``rhat_rank``), bulk and tail ESS with their windows, ``[n_groups,
    ld]``, each with an ``s2_`` twin without the last axis; padding is NaN / -1. ``z`` and ``z_folded`` (``[rows,
    n_chains, ld]``, with ``s2_z`` / ``s2_z_folded`` ``[rows, n_chains]``) are the rank-score chains, None unless
    asked for."""

    probs: np.ndarray
    tail: tuple
    max_lag: int
    arrays: dict
    z: Optional[np.ndarray] = None
    z_folded: Optional[np.ndarray] = None
    s2_z: Optional[np.ndarray] = None
    s2_z_folded: Optional[np.ndarray] = None
    n_rows: int = 0
    kernel_ms: float = 0.0
    rank_ms: float = 0.0

    def __getattr__(self, name):
        arrays = self.__dict__.get("arrays")
        if arrays is not None and name in arrays:
            return arrays[name]
        raise AttributeError(name)

    @classmethod
    def empty(cls, n_groups: int, ld: int, probs=(0.025, 0.5, 0.975), tail=(0.05, 0.95), max_lag: int = 0,
              scores=None) -> "ChainRank":
        """``scores``: None, or ``(rows, n_chains, with_s2)`` to hold the rank-score chains."""
        pr = quant_probs(probs)
        if len(tail) != 2 or not (0.0 < float(tail[0]) < float(tail[1]) < 1.0):
            raise ValueError("tail must be (lo, hi) with 0 < lo < hi < 1")
        if int(max_lag) != max_lag or int(max_lag) < 0:
            raise ValueError("max_lag must be an integer >= 0")
        g = int(n_groups)
        a = {}
        for f in _lib.CHAINRANK_DOUBLES:
            mid = {"q": (pr.size,), "q_tail": (2,)}.get(f, ())
            a[f] = np.full((g,) + mid + (ld,), np.nan)
            a["s2_" + f] = np.full((g,) + mid, np.nan)
        for f in _lib.CHAINRANK_WINDOWS:
            a[f] = np.full((g, ld), -1, np.int32)
            a["s2_" + f] = np.full((g,), -1, np.int32)
        cr = cls(pr, (float(tail[0]), float(tail[1])), int(max_lag), a)
        if scores is not None:
            rows, n, with_s2 = scores
            cr.z, cr.z_folded = np.full((rows, n, ld), np.nan), np.full((rows, n, ld), np.nan)
            if with_s2:
                cr.s2_z, cr.s2_z_folded = np.full((rows, n), np.nan), np.full((rows, n), np.nan)
        return cr

    def options(self) -> "_lib.tci_chainrank_options":
        o = _lib.tci_chainrank_options()
        o.nq = int(self.probs.size)
        for k, p in enumerate(self.probs):
            o.probs[k] = float(p)
        o.tail_lo, o.tail_hi = self.tail
        o.max_lag, o.flags = self.max_lag, 0
        return o

    def to_c(self) -> "_lib.tci_chainrank_outputs":
        out = _lib.tci_chainrank_outputs()
        for f in _lib.CHAINRANK_DOUBLES:
            setattr(out, f, _lib.ptr(self.arrays[f], _lib._dp))
            setattr(out, "s2_" + f, _lib.ptr(self.arrays["s2_" + f], _lib._dp))
        for f in _lib.CHAINRANK_WINDOWS:
            setattr(out, f, _lib.ptr(self.arrays[f], _lib._i32p))
            setattr(out, "s2_" + f, _lib.ptr(self.arrays["s2_" + f], _lib._i32p))
        for f in ("z", "z_folded", "s2_z", "s2_z_folded"):
            setattr(out, f, _lib.ptr(getattr(self, f), _lib._dp))
        return out

    def taken(self, out) -> "ChainRank":
        self.n_rows, self.kernel_ms, self.rank_ms = int(out.n_rows), float(out.kernel_ms), float(out.rank_ms)
        return self


FITCHECK_POINTWISE = ("lppd_i", "p_waic_i", "pit", "resid", "zbar", "z2")


def fitcheck_levels(levels) -> np.ndarray:
    """``levels`` as the float64 vector ``tci_fitcheck_options`` takes; ValueError outside its rules."""
    lv = np.ascontiguousarray(np.atleast_1d(levels), np.float64)
    if lv.ndim != 1 or not 1 <= len(lv) <= 8:
        raise ValueError("levels must hold 1 to 8 interval levels")
    if not np.all((lv > 0) & (lv < 1)):
        raise ValueError("levels must be strictly inside (0, 1)")
    return lv


@dataclasses.dataclass
class FitCheck:
    """Posterior predictive fit checks (``tci_fitcheck_outputs``; formulas in ``include/tci.h``). Pointwise, each
    ``[n_sel, 2, ld_out]`` with dye 0 = MS2 and 1 = PP7, NaN at unscored points and past a cell's N: ``lppd_i``,
    ``p_waic_i``, ``pit``, ``resid``, ``zbar``, ``z2``. Per cell ``[n_sel]``: ``n_obs`` (int32), ``lppd``, ``p_waic``,
    ``elpd_waic`` (WAIC = -2 x this), ``chi2``; ``coverage`` ``[n_sel, n_levels]`` at ``levels``; ``dw`` ``[n_sel, 2]``."""

    lppd_i: np.ndarray
    p_waic_i: np.ndarray
    pit: np.ndarray
    resid: np.ndarray
    zbar: np.ndarray
    z2: np.ndarray
    n_obs: np.ndarray
    lppd: np.ndarray
    p_waic: np.ndarray
    elpd_waic: np.ndarray
    chi2: np.ndarray
    coverage: np.ndarray
    dw: np.ndarray
    levels: np.ndarray
    n_samples: int = 0
    kernel_ms: float = 0.0    # device time of the fit-check kernel
    forward_ms: float = 0.0   # device time of the forward launches before it

    @classmethod
    def empty(cls, n: int, ld_out: int, levels=(0.5, 0.95), n_samples: int = 0) -> "FitCheck":
        lv = fitcheck_levels(levels)
        d = lambda *s: np.full(s, np.nan)  # noqa: E731
        return cls(*[d(n, 2, ld_out) for _ in FITCHECK_POINTWISE], np.zeros(n, np.int32), d(n), d(n), d(n), d(n),
                   d(n, len(lv)), d(n, 2), lv, int(n_samples))

    def options(self, scratch_bytes: int = 0) -> "_lib.tci_fitcheck_options":
        lv = (C.c_double * 8)(*self.levels)
        return _lib.tci_fitcheck_options(int(scratch_bytes), len(self.levels), lv)

    def to_c(self) -> "_lib.tci_fitcheck_outputs":
        P = lambda a: _lib.ptr(a, _lib._dp)  # noqa: E731
        return _lib.tci_fitcheck_outputs(*[P(getattr(self, f)) for f in FITCHECK_POINTWISE],
                                         _lib.ptr(self.n_obs, _lib._i32p), P(self.lppd), P(self.p_waic),
                                         P(self.elpd_waic), P(self.chi2), P(self.coverage), P(self.dw), 0.0, 0.0)


def loocheck_tail(S: int):
    """The tail length ``M = min(floor(S / 5), ceil(3 sqrt(S)))`` and the profile's point count
    ``G = 30 + floor(sqrt(M))`` of ``tci_loocheck`` for ``S`` samples; ValueError outside [32, 4096]."""
    S = int(S)
    if not 32 <= S <= 4096:
        raise ValueError(f"S = {S} must be in [32, 4096]")
    M = min(S // 5, int(math.ceil(3.0 * math.sqrt(float(S)))))
    return M, 30 + int(math.floor(math.sqrt(float(M))))


def loocheck_threshold(S: int) -> float:
    """The default ``khat_threshold`` for ``S`` samples: ``min(1 - 1 / log10(S), 0.7)``."""
    return min(1.0 - 1.0 / math.log10(float(S)), 0.7)


@dataclasses.dataclass
class LooCheck:
    """PSIS-LOO per chain and stacking weights per group (``tci_loocheck_outputs``; formulas in ``include/tci.h``).
    Pointwise, each ``[n_sel, 2, ld_out]`` with dye 0 = MS2 and 1 = PP7, NaN at unscored points and past a cell's N:
    ``elpd_loo_i``, ``lppd_i``, ``p_loo_i``, ``khat_i`` (+Inf: a degenerate tail). Per chain ``[n_sel]``: ``n_obs``,
    ``n_khat_bad`` (int32), ``elpd_loo``, ``p_loo``, ``lppd``, ``khat_max``, and ``weight`` (NaN for a chain in no
    group). Per group ``[n_groups]``: ``elpd_stack``, ``n_points``, ``n_iter`` (int32)."""

    elpd_loo_i: np.ndarray
    lppd_i: np.ndarray
    p_loo_i: np.ndarray
    khat_i: np.ndarray
    n_obs: np.ndarray
    elpd_loo: np.ndarray
    p_loo: np.ndarray
    lppd: np.ndarray
    khat_max: np.ndarray
    n_khat_bad: np.ndarray
    weight: np.ndarray
    elpd_stack: np.ndarray
    n_points: np.ndarray
    n_iter: np.ndarray
    n_samples: int = 0
    khat_threshold: float = float("nan")
    kernel_ms: float = 0.0    # device time of the loocheck kernel
    forward_ms: float = 0.0   # device time of the forward launches before it

    @classmethod
    def empty(cls, n: int, ld_out: int, n_groups: int = 0, n_samples: int = 0) -> "LooCheck":
        d = lambda *s: np.full(s, np.nan)  # noqa: E731
        z = lambda m: np.zeros(m, np.int32)  # noqa: E731
        g = int(n_groups)
        return cls(*[d(n, 2, ld_out) for _ in _lib.LOOCHECK_POINTWISE], z(n), *[d(n) for _ in _lib.LOOCHECK_SCALARS],
                   z(n), d(n), d(g), z(g), z(g), int(n_samples))

    def to_c(self) -> "_lib.tci_loocheck_outputs":
        P = lambda a: _lib.ptr(a, _lib._dp)  # noqa: E731
        I = lambda a: _lib.ptr(a, _lib._i32p)  # noqa: E731,E741
        return _lib.tci_loocheck_outputs(*[P(getattr(self, f)) for f in _lib.LOOCHECK_POINTWISE], I(self.n_obs),
                                         *[P(getattr(self, f)) for f in _lib.LOOCHECK_SCALARS], I(self.n_khat_bad),
                                         P(self.weight), P(self.elpd_stack), I(self.n_points), I(self.n_iter),
                                         0.0, 0.0, 0.0)


@dataclasses.dataclass
class ChainLp:
    """Log-posterior trace, best sample and DIC of every chain (``tci_chainlp_outputs``; formulas in
    ``include/tci.h``). Traces ``[n_rows, n_chains]``: ``ss`` (mcmcstat's ``sschain``), ``pri``, ``dev``, ``lp``.
    Per chain ``[n_chains]``: the scalars of ``_lib.CHAINLP_SCALARS`` and ``best_row`` (int64, -1 for a chain with a
    non-finite trace value); ``theta_best`` and ``theta_mean`` ``[n_chains, ld]``, padding NaN."""

    ss: np.ndarray
    pri: np.ndarray
    dev: np.ndarray
    lp: np.ndarray
    ss_min: np.ndarray
    ss_mean: np.ndarray
    dev_mean: np.ndarray
    dev_var: np.ndarray
    lp_best: np.ndarray
    ss_best: np.ndarray
    s2_best: np.ndarray
    s2_mean: np.ndarray
    ss_hat: np.ndarray
    d_hat: np.ndarray
    p_d: np.ndarray
    p_v: np.ndarray
    dic: np.ndarray
    best_row: np.ndarray
    theta_best: np.ndarray
    theta_mean: np.ndarray
    n_rows: int = 0
    kernel_ms: float = 0.0

    @classmethod
    def empty(cls, rows: int, n: int, ld: int) -> "ChainLp":
        d = lambda *s: np.full(s, np.nan)  # noqa: E731
        return cls(*[d(rows, n) for _ in _lib.CHAINLP_TRACES], *[d(n) for _ in _lib.CHAINLP_SCALARS],
                   np.full(n, -1, np.int64), d(n, ld), d(n, ld))

    def options(self) -> "_lib.tci_chainlp_options":
        return _lib.tci_chainlp_options(0)

    def to_c(self) -> "_lib.tci_chainlp_outputs":
        P = lambda a: _lib.ptr(a, _lib._dp)  # noqa: E731
        return _lib.tci_chainlp_outputs(*[P(getattr(self, f)) for f in _lib.CHAINLP_TRACES + _lib.CHAINLP_SCALARS],
                                        _lib.ptr(self.best_row, _lib._i64p), P(self.theta_best), P(self.theta_mean),
                                        0, 0.0)


@dataclasses.dataclass
class ModeSearch:
    """The final population of a mode search and its best member per cell (``tci_modesearch_outputs``; the definition is
    in ``include/tci.h``). ``pop`` ``[n_sel, n_pop, ld]`` with ``f`` and ``ss`` ``[n_sel, n_pop]``; per cell ``[n_sel]``:
    ``best`` (int32, the least index of the least ``f``), ``f_best``, ``ss_best``, ``pri_best`` and ``theta_best``
    ``[n_sel, ld]`` (padding NaN); ``f_trace`` ``[n_gen + 1, n_sel]``: the least ``f`` after each generation, row 0 the
    initial population's; ``n_accepted`` ``[n_gen, n_sel]`` (int32)."""

    pop: np.ndarray
    f: np.ndarray
    ss: np.ndarray
    best: np.ndarray
    theta_best: np.ndarray
    f_best: np.ndarray
    ss_best: np.ndarray
    pri_best: np.ndarray
    f_trace: np.ndarray
    n_accepted: np.ndarray
    n_gen: int = 0
    n_evals: int = 0
    kernel_ms: float = 0.0

    @classmethod
    def empty(cls, n: int, n_pop: int, ld: int, n_gen: int) -> "ModeSearch":
        d = lambda *s: np.full(s, np.nan)  # noqa: E731
        return cls(d(n, n_pop, ld), d(n, n_pop), d(n, n_pop), np.full(n, -1, np.int32), d(n, ld), d(n), d(n), d(n),
                   d(n_gen + 1, n), np.zeros((n_gen, n), np.int32), int(n_gen))

    def to_c(self) -> "_lib.tci_modesearch_outputs":
        P = lambda a: _lib.ptr(a, _lib._dp)  # noqa: E731
        I = lambda a: _lib.ptr(a, _lib._i32p)  # noqa: E731
        return _lib.tci_modesearch_outputs(P(self.pop), P(self.f), P(self.ss), I(self.best), P(self.theta_best),
                                           P(self.f_best), P(self.ss_best), P(self.pri_best), P(self.f_trace),
                                           I(self.n_accepted) if self.n_gen else None, 0, 0.0)


@dataclasses.dataclass
class Demc:
    """A DE-MC run (``tci_demc_outputs``; the definition is in ``include/tci.h``). Member ``i`` of selected cell ``k``
    is chain ``k * n_pop + i``. ``chain`` ``[n_keep, n_chains, ld]`` with ``s2chain``, ``sschain`` and ``prichain``
    ``[n_keep, n_chains]``: the states after generations 0, thin, 2 thin, ..; ``pop`` ``[n_sel, n_pop, ld]``, ``s2`` and
    ``ss`` ``[n_sel, n_pop]``: the final population; per member ``accept_rate``, ``n_oob`` (int32) and ``n_evals``
    (int64) ``[n_sel, n_pop]``; the logs ``logr``, ``accepted`` and ``trial_oob`` (uint8) ``[log_rows, n_chains]``, row
    ``g - 1`` for generation ``g``; ``rhat`` / ``ess`` / ``rank``: the group reductions over the cells' members, or None."""

    chain: np.ndarray
    s2chain: np.ndarray
    sschain: np.ndarray
    prichain: np.ndarray
    pop: np.ndarray
    s2: np.ndarray
    ss: np.ndarray
    accept_rate: np.ndarray
    n_oob: np.ndarray
    n_evals: np.ndarray
    logr: np.ndarray
    accepted: np.ndarray
    trial_oob: np.ndarray
    n_gen: int = 0
    thin: int = 0
    kernel_ms: float = 0.0
    rhat: Optional[ChainRhat] = None
    ess: Optional[ChainEss] = None
    rank: Optional["ChainRank"] = None

    @classmethod
    def empty(cls, n: int, n_pop: int, ld: int, n_gen: int, thin: int, log_rows: int) -> "Demc":
        d = lambda *s: np.full(s, np.nan)  # noqa: E731
        K = n_gen // thin + 1 if thin > 0 else 0
        B, G = n * n_pop, min(int(log_rows), int(n_gen))
        return cls(d(K, B, ld), d(K, B), d(K, B), d(K, B), d(n, n_pop, ld), d(n, n_pop), d(n, n_pop), d(n, n_pop),
                   np.zeros((n, n_pop), np.int32), np.zeros((n, n_pop), np.int64), d(G, B), np.zeros((G, B), np.uint8),
                   np.zeros((G, B), np.uint8), int(n_gen), int(thin))

    def to_c(self) -> "_lib.tci_demc_outputs":
        P = lambda a: _lib.ptr(a, _lib._dp) if a.size else None  # noqa: E731
        U = lambda a: _lib.ptr(a, _lib._u8p) if a.size else None  # noqa: E731
        return _lib.tci_demc_outputs(P(self.chain), P(self.s2chain), P(self.sschain), P(self.prichain), P(self.pop),
                                     P(self.s2), P(self.ss), P(self.accept_rate), _lib.ptr(self.n_oob, _lib._i32p),
                                     _lib.ptr(self.n_evals, _lib._i64p), P(self.logr), U(self.accepted),
                                     U(self.trial_oob), self.logr.shape[0], 0, 0.0)


@dataclasses.dataclass
class DemcZs(Demc):
    """A DE-MC(zs) run (``tci_demczs_outputs``; the definition is in ``include/tci.h``): :class:`Demc`'s fields, with
    ``trial_oob`` 2 for a null snooker move, plus ``n_null`` (int32) ``[n_sel, n_pop]``, the logs ``ljac`` and
    ``snooker`` (uint8) ``[log_rows, n_chains]``, and ``archive`` ``[n_sel, n_archive, ld]`` (None unless asked for):
    ``z0`` followed by the chains' states at the append generations. ``m0``: the rows of ``z0``.
    ``bounds`` (``'reject'`` or ``'reflect'``) and ``census``: what the run was asked for (``tci_demczs_run_bounds``).
    With ``census``: ``n_cross``, ``oob_lo`` and ``oob_hi`` (int32) ``[n_sel, n_pop, ld]``, -1 at ``j >= P``, and the log
    ``n_left`` (int32) ``[log_rows, n_chains]``. With ``bounds='reflect'``: the log ``n_refl`` (int32), ``n_reflected``
    (int32) ``[n_sel, n_pop]`` and ``orient`` (uint8) ``[n_sel, n_pop, ld]``. Each is None when its feature is off."""

    n_null: Optional[np.ndarray] = None
    ljac: Optional[np.ndarray] = None
    snooker: Optional[np.ndarray] = None
    archive: Optional[np.ndarray] = None
    n_archive: int = 0
    m0: int = 0
    bounds: str = "reject"
    census: bool = False
    n_cross: Optional[np.ndarray] = None
    oob_lo: Optional[np.ndarray] = None
    oob_hi: Optional[np.ndarray] = None
    n_left: Optional[np.ndarray] = None
    n_refl: Optional[np.ndarray] = None
    n_reflected: Optional[np.ndarray] = None
    orient: Optional[np.ndarray] = None

    @classmethod
    def empty_zs(cls, n: int, n_pop: int, ld: int, n_gen: int, thin: int, log_rows: int, m0: int, append_every: int,
                 archive: bool) -> "DemcZs":
        base = Demc.empty(n, n_pop, ld, n_gen, thin, log_rows)
        G, B = base.logr.shape
        M = int(m0) + n_pop * (int(n_gen) // max(int(append_every), 1))
        return cls(**{f.name: getattr(base, f.name) for f in dataclasses.fields(Demc)},
                   n_null=np.zeros((n, n_pop), np.int32), ljac=np.full((G, B), np.nan), snooker=np.zeros((G, B), np.uint8),
                   archive=np.full((n, M, ld), np.nan) if archive else None, n_archive=M, m0=int(m0))

    def to_c(self) -> "_lib.tci_demczs_outputs":
        base = Demc.to_c(self)
        P = lambda a: _lib.ptr(a, _lib._dp) if a is not None and a.size else None  # noqa: E731
        return _lib.tci_demczs_outputs(*[getattr(base, f) for f, _ in _lib.tci_demc_outputs._fields_],
                                       _lib.ptr(self.n_null, _lib._i32p), P(self.ljac),
                                       _lib.ptr(self.snooker, _lib._u8p) if self.snooker.size else None, P(self.archive), 0)

    def with_bounds(self, bounds: str, census: bool) -> "_lib.tci_bounds_outputs":
        """Allocate the outputs of the features that are on, and return them as ``tci_bounds_outputs``."""
        n, n_pop, ld = self.pop.shape
        G, B = self.logr.shape
        self.bounds, self.census = bounds, bool(census)
        full = lambda: np.full((n, n_pop, ld), -1, np.int32)  # noqa: E731
        if census:
            self.n_cross, self.oob_lo, self.oob_hi = full(), full(), full()
            self.n_left = np.full((G, B), -1, np.int32)
        if bounds == "reflect":
            self.n_refl = np.zeros((G, B), np.int32)
            self.n_reflected = np.zeros((n, n_pop), np.int32)
            self.orient = np.zeros((n, n_pop, ld), np.uint8)
        I = lambda a: _lib.ptr(a, _lib._i32p) if a is not None and a.size else None  # noqa: E731, E741
        return _lib.tci_bounds_outputs(I(self.n_cross), I(self.oob_lo), I(self.oob_hi), I(self.n_left), I(self.n_refl),
                                       I(self.n_reflected), _lib.ptr(self.orient, _lib._u8p))


class Likelihood:
    """SS evaluator bound to one device and one dataset (the C ``tci_ctx``)."""

    def __init__(self, cells: Cells, construct="P2P-MS2v5-LacZ-PP7v4", device: int = 0,
                 lib_path: Optional[str] = None):
        self._lib = _lib.load(lib_path)  # lib_path: an A/B build variant (default: libtci.so)
        self.cells = cells
        self.construct: Construct = as_construct(construct)
        self.device = int(device)
        cs, self._cs_arrays = self.construct.to_c()
        self._cells_c = _lib.tci_cells(cells.n_cells, _lib.ptr(cells.offsets, _lib._i64p), _lib.ptr(cells.t, _lib._dp),
                                       _lib.ptr(cells.ms2, _lib._dp), _lib.ptr(cells.pp7, _lib._dp))
        h = C.c_void_p()
        rc = self._lib.tci_create(C.byref(self._cells_c), C.byref(cs), self.device, C.byref(h))
        if rc != _lib.TCI_OK:
            msg = self._lib.tci_last_error(h).decode() if h.value else "tci_create failed"
            if h.value:
                self._lib.tci_destroy(h)
            raise _lib.TciError(rc, msg)
        self._h = h
        self.lengths = cells.lengths.astype(np.int64)

    # -- lifecycle ---------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.tci_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int):
        if rc != _lib.TCI_OK:
            raise _lib.TciError(rc, self._lib.tci_last_error(self._h).decode())

    @property
    def info(self) -> dict:
        i = _lib.tci_info()
        self._check(self._lib.tci_get_info(self._h, C.byref(i)))
        return {k: getattr(i, k) for k, _ in i._fields_}

    def set_force_exact(self, scan: bool = False, positions: bool = False):
        """Test hook: force the exact serial counter scan and/or the exact position sweep."""
        self._check(self._lib.tci_set_force_exact_scan(self._h, int(bool(scan)) | (int(bool(positions)) << 1)))

    def grid(self, cell: int) -> np.ndarray:
        m = C.c_int64()
        out = np.empty(int(self.lengths[cell]))
        self._check(self._lib.tci_cell_grid(self._h, int(cell), _lib.ptr(out, _lib._dp), len(out), C.byref(m)))
        return out[: m.value]

    # -- evaluation (host arrays, synchronous) -----------------------------
    def ss_batch(self, theta: np.ndarray, cell_id: Sequence[int], active: Optional[np.ndarray] = None) -> np.ndarray:
        """``ss[b] = ssfun(theta[b], cell[cell_id[b]])``; inactive rows -> +Inf."""
        theta = np.ascontiguousarray(np.atleast_2d(theta), np.float64)
        cid = np.ascontiguousarray(cell_id, np.int32)
        B, ld = theta.shape
        if len(cid) != B:
            raise ValueError("cell_id must have one entry per theta row")
        act = None if active is None else np.ascontiguousarray(active, np.uint8)
        if act is not None and len(act) != B:
            raise ValueError("active must have one entry per theta row")
        out = np.empty(B)
        self._check(self._lib.tci_ss_batch(self._h, _lib.ptr(theta, _lib._dp), ld, _lib.ptr(cid, _lib._i32p),
                                           _lib.ptr(act, _lib._u8p), B, _lib.ptr(out, _lib._dp)))
        return out

    def ssfun(self, theta: np.ndarray, cell: int) -> float:
        """One ``ssfun(theta, data)`` call for one cell."""
        th = np.ascontiguousarray(theta, np.float64)
        out = np.empty(1)
        self._check(self._lib.tci_ssfun(self._h, int(cell), _lib.ptr(th, _lib._dp), len(th), _lib.ptr(out, _lib._dp)))
        return float(out[0])

    def forward(self, theta: np.ndarray, cell_id: Sequence[int], grid: str = "interp"):
        """Simulated (MS2, PP7) at each row's acquisition times, shape (B, max N); NaN-padded.
        ``grid='raw'``: forward model on the raw times (TranscriptionCycleMCMC.m:307-309);
        ``grid='interp'``: through the uniform grid + interp1, as inside the SS."""
        mode = {"interp": _lib.TCI_GRID_INTERP, "raw": _lib.TCI_GRID_RAW}[grid]
        theta = np.ascontiguousarray(np.atleast_2d(theta), np.float64)
        cid = np.ascontiguousarray(cell_id, np.int32)
        B, ld = theta.shape
        ld_out = int(self.lengths[cid].max()) if B else 1
        ms2 = np.full((B, ld_out), np.nan)
        pp7 = np.full((B, ld_out), np.nan)
        self._check(self._lib.tci_forward(self._h, _lib.ptr(theta, _lib._dp), ld, _lib.ptr(cid, _lib._i32p), B, mode,
                                          _lib.ptr(ms2, _lib._dp), _lib.ptr(pp7, _lib._dp), ld_out))
        return ms2, pp7

    def predict(self, theta: np.ndarray, cell_id: Sequence[int], probs=(0.025, 0.5, 0.975), grid: str = "raw",
                scratch_bytes: int = 0):
        """Posterior predictive bands (mcmcstat's ``mcmcpred`` / ``plims``) reduced on the device
        (``tci_predict``): ``theta`` is ``[n_sel, S, ld]``, S posterior samples of cell ``cell_id[k]``
        each. Returns ``ms2_q, pp7_q`` shaped ``[n_sel, nq, max N]``: at every acquisition time the
        ``probs`` quantiles over the S simulated values, ``interp1(sort(x), (S-1)*p+1)`` with NaN
        sorted last; NaN past a cell's N. ``scratch_bytes``: cap on the device scratch holding the
        simulated rows (0 = 1 GiB); beyond it whole cells go in chunks, with the same results."""
        if grid not in ("interp", "raw"):
            raise ValueError(f"grid must be 'raw' or 'interp', got {grid!r}")
        theta = np.ascontiguousarray(theta, np.float64)
        if theta.ndim != 3:
            raise ValueError("theta must be [n_sel, S, ld]: S posterior samples per selected cell")
        cid = np.ascontiguousarray(cell_id, np.int32)
        n_sel, S, ld = theta.shape
        if cid.shape != (n_sel,):
            raise ValueError("cell_id must have one entry per selected cell (theta.shape[0])")
        pr = np.ascontiguousarray(np.atleast_1d(probs), np.float64)
        if pr.ndim != 1 or not 1 <= len(pr) <= 16:
            raise ValueError("probs must hold 1 to 16 probabilities")
        if not np.all((pr >= 0) & (pr <= 1)):
            raise ValueError("probs must be finite and in [0, 1]")
        if not 1 <= S <= 4096:
            raise ValueError(f"S = theta.shape[1] = {S} must be in [1, 4096]")
        if int(scratch_bytes) < 0:
            raise ValueError("scratch_bytes must be >= 0")
        if n_sel and (cid.min() < 0 or cid.max() >= len(self.lengths)):
            raise ValueError("cell_id out of range")
        ld_out = int(self.lengths[cid].max()) if n_sel else 1
        nq = len(pr)
        ms2 = np.full((n_sel, nq, ld_out), np.nan)
        pp7 = np.full((n_sel, nq, ld_out), np.nan)
        opt = _lib.tci_predict_options({"interp": _lib.TCI_GRID_INTERP, "raw": _lib.TCI_GRID_RAW}[grid],
                                       int(scratch_bytes))
        self._check(self._lib.tci_predict(self._h, C.byref(opt), _lib.ptr(theta, _lib._dp), ld,
                                          _lib.ptr(cid, _lib._i32p), n_sel, S, _lib.ptr(pr, _lib._dp), nq,
                                          _lib.ptr(ms2, _lib._dp), _lib.ptr(pp7, _lib._dp), ld_out))
        return ms2, pp7

    def fitcheck(self, theta: np.ndarray, s2: np.ndarray, cell_id: Sequence[int], levels=(0.5, 0.95),
                 scratch_bytes: int = 0) -> FitCheck:
        """Posterior predictive fit checks reduced on the device (``tci_fitcheck``; formulas in
        ``include/tci.h``): ``theta`` is ``[n_sel, S, ld]``, S posterior samples of cell ``cell_id[k]`` each, and
        ``s2`` ``[n_sel, S]`` the sigma2 of the same chain rows (finite and > 0). Every datum of the cell is scored
        under the Gaussian mixture the samples define, with the forward model through the uniform grid + interp1 as
        inside the SS. Returns a :class:`FitCheck`; ``levels``: 1 to 8 central-interval levels inside (0, 1) for
        ``coverage``; ``scratch_bytes`` as in :meth:`predict`."""
        theta = np.ascontiguousarray(theta, np.float64)
        if theta.ndim != 3:
            raise ValueError("theta must be [n_sel, S, ld]: S posterior samples per selected cell")
        cid = np.ascontiguousarray(cell_id, np.int32)
        n_sel, S, ld = theta.shape
        if cid.shape != (n_sel,):
            raise ValueError("cell_id must have one entry per selected cell (theta.shape[0])")
        s2 = np.ascontiguousarray(s2, np.float64)
        if s2.shape != (n_sel, S):
            raise ValueError("s2 must be [n_sel, S]: one sigma2 per theta row")
        if not np.all(np.isfinite(s2) & (s2 > 0)):
            raise ValueError("s2 must be finite and > 0")
        lv = fitcheck_levels(levels)
        if not 1 <= S <= 4096:
            raise ValueError(f"S = theta.shape[1] = {S} must be in [1, 4096]")
        if int(scratch_bytes) < 0:
            raise ValueError("scratch_bytes must be >= 0")
        if n_sel and (cid.min() < 0 or cid.max() >= len(self.lengths)):
            raise ValueError("cell_id out of range")
        ld_out = int(self.lengths[cid].max()) if n_sel else 1
        fc = FitCheck.empty(n_sel, ld_out, lv, S)
        opt, out = fc.options(scratch_bytes), fc.to_c()
        self._check(self._lib.tci_fitcheck(self._h, C.byref(opt), _lib.ptr(theta, _lib._dp), ld, _lib.ptr(s2, _lib._dp),
                                           _lib.ptr(cid, _lib._i32p), n_sel, S, ld_out, C.byref(out)))
        fc.kernel_ms, fc.forward_ms = float(out.kernel_ms), float(out.forward_ms)
        return fc

    def loocheck(self, theta: np.ndarray, s2: np.ndarray, cell_id: Sequence[int], group=None,
                 khat_threshold: Optional[float] = None, max_iter: int = 5000, tol: float = 1e-12,
                 scratch_bytes: int = 0) -> LooCheck:
        """PSIS-LOO of every selected chain and stacking weights across the chains of a group, reduced on the device
        (``tci_loocheck``; formulas in ``include/tci.h``). ``theta``, ``s2`` and ``cell_id`` as in :meth:`fitcheck`,
        one entry per selected chain, with 32 <= S <= 4096. ``group``: None (no groups) or one integer id per chain,
        -1 = no group; the chains of a group must select one cell and get the simplex ``weight`` that maximises the
        stacked leave-one-out density. ``khat_threshold``: the Pareto k above which a point counts into
        ``n_khat_bad`` (None: ``min(1 - 1 / log10(S), 0.7)``); ``max_iter``, ``tol``: the stopping rule of the
        weight iteration. Returns a :class:`LooCheck`."""
        theta = np.ascontiguousarray(theta, np.float64)
        if theta.ndim != 3:
            raise ValueError("theta must be [n_sel, S, ld]: S posterior samples per selected chain")
        cid = np.ascontiguousarray(cell_id, np.int32)
        n_sel, S, ld = theta.shape
        if cid.shape != (n_sel,):
            raise ValueError("cell_id must have one entry per selected chain (theta.shape[0])")
        s2 = np.ascontiguousarray(s2, np.float64)
        if s2.shape != (n_sel, S):
            raise ValueError("s2 must be [n_sel, S]: one sigma2 per theta row")
        if not np.all(np.isfinite(s2) & (s2 > 0)):
            raise ValueError("s2 must be finite and > 0")
        if not 32 <= S <= 4096:
            raise ValueError(f"S = theta.shape[1] = {S} must be in [32, 4096]")
        if int(scratch_bytes) < 0:
            raise ValueError("scratch_bytes must be >= 0")
        if int(max_iter) != max_iter or int(max_iter) < 1:
            raise ValueError("max_iter must be an integer >= 1")
        if not (np.isfinite(tol) and tol >= 0):
            raise ValueError("tol must be finite and >= 0")
        if khat_threshold is not None and not (np.isfinite(khat_threshold) and khat_threshold > 0):
            raise ValueError("khat_threshold must be finite and > 0")
        if n_sel and (cid.min() < 0 or cid.max() >= len(self.lengths)):
            raise ValueError("cell_id out of range")
        g, n_groups = None, 0
        if group is not None and n_sel:
            g, n_groups = rhat_groups(group, n_sel)
            for k in np.unique(g[g >= 0]):
                if len(np.unique(cid[g == k])) > 1:
                    raise ValueError(f"group {int(k)} selects more than one cell")
        ld_out = int(self.lengths[cid].max()) if n_sel else 1
        lc = LooCheck.empty(n_sel, ld_out, n_groups, S)
        opt = _lib.tci_loocheck_options(int(scratch_bytes), n_groups, 0.0 if khat_threshold is None else
                                        float(khat_threshold), int(max_iter), float(tol))
        out = lc.to_c()
        self._check(self._lib.tci_loocheck(self._h, C.byref(opt), _lib.ptr(theta, _lib._dp), ld, _lib.ptr(s2, _lib._dp),
                                           _lib.ptr(cid, _lib._i32p), _lib.ptr(g, _lib._i32p), n_sel, S, ld_out,
                                           C.byref(out)))
        lc.khat_threshold = float(out.khat_threshold)
        lc.kernel_ms, lc.forward_ms = float(out.kernel_ms), float(out.forward_ms)
        return lc

    def chainstats(self, chain: np.ndarray, s2chain: Optional[np.ndarray] = None, npar=None, max_lag: int = 0):
        """Convergence diagnostics of a chain held on the host (mcmcstat's ``chainstats``), reduced
        on the device (``tci_chainstats``; formulas in ``include/tci.h``). ``chain`` is
        ``[rows, n_chains, ld]`` (a 2-D ``[rows, ld]`` array is one chain), ``s2chain`` ``[rows, n_chains]``
        or None, ``npar`` the number of real columns per chain (None: ``ld``); ``max_lag``: most lags the
        autocorrelation time may use (0 = rows). Returns a :class:`ChainStats`; padding is NaN
        (window -1), and so is every statistic of a column holding a non-finite value."""
        chain = np.asarray(chain, np.float64)
        if chain.ndim == 2:
            chain = chain[:, None, :]
        if chain.ndim != 3:
            raise ValueError("chain must be [rows, n_chains, ld]")
        chain = np.ascontiguousarray(chain)
        rows, n, ld = chain.shape
        s2 = None
        if s2chain is not None:
            s2 = np.ascontiguousarray(np.asarray(s2chain, np.float64).reshape(rows, n))
        npr = None
        if npar is not None:
            npr = np.ascontiguousarray(np.broadcast_to(np.asarray(npar, np.int32), (n,)))
        st = ChainStats.empty(n, ld)
        opt = _lib.tci_chainstats_options(int(max_lag))
        out = st.to_c()
        self._check(self._lib.tci_chainstats(self._h, C.byref(opt), _lib.ptr(chain, _lib._dp), _lib.ptr(s2, _lib._dp),
                                             rows, n, ld, _lib.ptr(npr, _lib._i32p), C.byref(out)))
        st.n_rows, st.kernel_ms = int(out.n_rows), float(out.kernel_ms)
        return st

    def chaincov(self, chain: np.ndarray, npar=None, scratch_bytes: int = 0) -> ChainCov:
        """Mean, covariance and correlation of every chain held on the host (MATLAB's ``mean(chain)``,
        ``cov(chain)``, ``corrcoef(chain)``), reduced on the device (``tci_chaincov``; formulas in
        ``include/tci.h``). ``chain`` and ``npar`` as in :meth:`chainstats`; at least 2 rows.
        ``scratch_bytes``: cap on the device buffer for the matrices (0 = 1 GiB); past it the chains go
        through in groups, with the same bits. Returns a :class:`ChainCov`; padding is NaN, and so are the
        mean, row and column of a column holding a non-finite value."""
        chain = np.asarray(chain, np.float64)
        if chain.ndim == 2:
            chain = chain[:, None, :]
        if chain.ndim != 3:
            raise ValueError("chain must be [rows, n_chains, ld]")
        chain = np.ascontiguousarray(chain)
        rows, n, ld = chain.shape
        npr = None
        if npar is not None:
            npr = np.ascontiguousarray(np.broadcast_to(np.asarray(npar, np.int32), (n,)))
        cc = ChainCov.empty(n, ld)
        opt = _lib.tci_chaincov_options(int(scratch_bytes))
        out = cc.to_c()
        self._check(self._lib.tci_chaincov(self._h, C.byref(opt), _lib.ptr(chain, _lib._dp), rows, n, ld,
                                           _lib.ptr(npr, _lib._i32p), C.byref(out)))
        cc.n_rows, cc.kernel_ms = int(out.n_rows), float(out.kernel_ms)
        return cc

    def chainquant(self, chain: np.ndarray, s2chain: Optional[np.ndarray] = None, npar=None,
                   probs=(0.025, 0.5, 0.975)) -> ChainQuant:
        """Exact quantiles of every column of a chain held on the host (mcmcstat's ``plims(chain, probs)``:
        ``interp1(sort(x), (rows-1)*p+1)``), selected on the device (``tci_chainquant``; the definition is in
        ``include/tci.h``). ``chain``, ``s2chain`` and ``npar`` as in :meth:`chainstats`; ``probs``: 1 to 16
        probabilities in [0, 1]. Returns a :class:`ChainQuant`; padding is NaN, and so is every quantile of a
        column holding a non-finite value."""
        chain = np.asarray(chain, np.float64)
        if chain.ndim == 2:
            chain = chain[:, None, :]
        if chain.ndim != 3:
            raise ValueError("chain must be [rows, n_chains, ld]")
        chain = np.ascontiguousarray(chain)
        rows, n, ld = chain.shape
        s2 = None
        if s2chain is not None:
            s2 = np.ascontiguousarray(np.asarray(s2chain, np.float64).reshape(rows, n))
        npr = None
        if npar is not None:
            npr = np.ascontiguousarray(np.broadcast_to(np.asarray(npar, np.int32), (n,)))
        cq = ChainQuant.empty(n, ld, probs)
        opt, out = cq.options(), cq.to_c()
        self._check(self._lib.tci_chainquant(self._h, C.byref(opt), _lib.ptr(chain, _lib._dp), _lib.ptr(s2, _lib._dp),
                                             rows, n, ld, _lib.ptr(npr, _lib._i32p), C.byref(out)))
        cq.n_rows, cq.kernel_ms = int(out.n_rows), float(out.kernel_ms)
        return cq

    def chaindens(self, chain: np.ndarray, s2chain: Optional[np.ndarray] = None, npar=None, n_grid: int = 100,
                  n_bins: int = 20, bw_scale: float = 1.0) -> ChainDens:
        """Marginal density and histogram of every column of a chain held on the host (mcmcstat's ``density.m``
        Gaussian kernel estimate, as ``mcmcplot(chain, [], res, 'denspanel')`` draws it, and the ``histogram`` of
        the reference's ``ApproveMCMCResults``), reduced on the device (``tci_chaindens``; the definition and its
        two deviations from mcmcstat are in ``include/tci.h``). ``chain``, ``s2chain`` and ``npar`` as in
        :meth:`chainstats`; at least 2 rows. ``n_grid``: 2 to 256 density points per column over its range
        widened by 8 % each side; ``n_bins``: 1 to 256 equal bins over its range; ``bw_scale`` multiplies the
        rule-of-thumb bandwidth. Returns a :class:`ChainDens`; padding is NaN (counts -1), and so is a column
        holding a non-finite value; a constant column has bandwidth 0 and a NaN density."""
        chain = np.asarray(chain, np.float64)
        if chain.ndim == 2:
            chain = chain[:, None, :]
        if chain.ndim != 3:
            raise ValueError("chain must be [rows, n_chains, ld]")
        chain = np.ascontiguousarray(chain)
        rows, n, ld = chain.shape
        s2 = None
        if s2chain is not None:
            s2 = np.ascontiguousarray(np.asarray(s2chain, np.float64).reshape(rows, n))
        npr = None
        if npar is not None:
            npr = np.ascontiguousarray(np.broadcast_to(np.asarray(npar, np.int32), (n,)))
        cd = ChainDens.empty(n, ld, n_grid, n_bins, bw_scale)
        opt, out = cd.options(), cd.to_c()
        self._check(self._lib.tci_chaindens(self._h, C.byref(opt), _lib.ptr(chain, _lib._dp), _lib.ptr(s2, _lib._dp),
                                            rows, n, ld, _lib.ptr(npr, _lib._i32p), C.byref(out)))
        cd.n_rows, cd.kernel_ms = int(out.n_rows), float(out.kernel_ms)
        return cd

    def chainrhat(self, chain: np.ndarray, s2chain: Optional[np.ndarray] = None, npar=None, group=None) -> ChainRhat:
        """Gelman-Rubin's potential scale reduction factor across replicate chains held on the host (mcmcstat's
        ``psrf``), classic and split, with the pooled posterior mean and standard deviation, reduced on the device
        (``tci_chainrhat``; the definition is in ``include/tci.h``). ``chain``, ``s2chain`` and ``npar`` as in
        :meth:`chainstats`; ``group``: one id per chain, the chains of equal id form a group (taken in chain order),
        -1 = in no group; None = all chains form one group. The chains of a group must have one ``npar``. Returns a
        :class:`ChainRhat` of ``max id + 1`` groups; padding is NaN, and so is every output of a column holding a
        non-finite value in any chain of the group, and the classic factor of a group of one chain."""
        chain = np.asarray(chain, np.float64)
        if chain.ndim == 2:
            chain = chain[:, None, :]
        if chain.ndim != 3:
            raise ValueError("chain must be [rows, n_chains, ld]")
        chain = np.ascontiguousarray(chain)
        rows, n, ld = chain.shape
        s2 = None
        if s2chain is not None:
            s2 = np.ascontiguousarray(np.asarray(s2chain, np.float64).reshape(rows, n))
        npr = None
        if npar is not None:
            npr = np.ascontiguousarray(np.broadcast_to(np.asarray(npar, np.int32), (n,)))
        grp, ng = rhat_groups(group, n, npr)
        cr = ChainRhat.empty(ng, ld)
        opt, out = cr.options(), cr.to_c()
        self._check(self._lib.tci_chainrhat(self._h, C.byref(opt), _lib.ptr(chain, _lib._dp), _lib.ptr(s2, _lib._dp),
                                            rows, n, ld, _lib.ptr(npr, _lib._i32p), _lib.ptr(grp, _lib._i32p), ng,
                                            C.byref(out)))
        cr.n_rows, cr.kernel_ms = int(out.n_rows), float(out.kernel_ms)
        return cr

    def chainess(self, chain: np.ndarray, s2chain: Optional[np.ndarray] = None, npar=None, group=None,
                 max_lag: int = 0) -> ChainEss:
        """The multi-chain effective sample size of replicate chains held on the host (BDA3 11.5, Geyer's initial
        monotone sequence; the ``n_eff`` beside R-hat), classic and split, with its autocorrelation time, the lags
        summed and the pooled mean's Monte-Carlo standard error, reduced on the device (``tci_chainess``; the
        definition is in ``include/tci.h``). Arguments as in :meth:`chainrhat`; a group of one chain gives the
        single-chain estimate. ``max_lag``: cap on the lags (0 = none); a column the cap ends before its sequence
        stops has ``tau = inf`` and ``ess = 0``. Returns a :class:`ChainEss`; padding and columns with a non-finite
        entry are NaN / -1."""
        chain = np.asarray(chain, np.float64)
        if chain.ndim == 2:
            chain = chain[:, None, :]
        if chain.ndim != 3:
            raise ValueError("chain must be [rows, n_chains, ld]")
        chain = np.ascontiguousarray(chain)
        rows, n, ld = chain.shape
        s2 = None
        if s2chain is not None:
            s2 = np.ascontiguousarray(np.asarray(s2chain, np.float64).reshape(rows, n))
        npr = None
        if npar is not None:
            npr = np.ascontiguousarray(np.broadcast_to(np.asarray(npar, np.int32), (n,)))
        grp, ng = rhat_groups(group, n, npr)
        ce = ChainEss.empty(ng, ld, max_lag)
        opt, out = ce.options(), ce.to_c()
        self._check(self._lib.tci_chainess(self._h, C.byref(opt), _lib.ptr(chain, _lib._dp), _lib.ptr(s2, _lib._dp),
                                           rows, n, ld, _lib.ptr(npr, _lib._i32p), _lib.ptr(grp, _lib._i32p), ng,
                                           C.byref(out)))
        ce.n_rows, ce.kernel_ms = int(out.n_rows), float(out.kernel_ms)
        return ce

    def chainrank(self, chain: np.ndarray, s2chain: Optional[np.ndarray] = None, npar=None, group=None,
                  probs=(0.025, 0.5, 0.975), tail=(0.05, 0.95), max_lag: int = 0, scores: bool = False) -> ChainRank:
        """Rank-normalised split R-hat (bulk and folded), bulk and tail effective sample size and the pooled quantiles
        of replicate chains held on the host (Vehtari, Gelman, Simpson, Carpenter and Buerkner 2021), from one pooled
        sort of every group's column on the device (``tci_chainrank``; the definition is in ``include/tci.h``).
        Arguments as in :meth:`chainess`; ``probs``: 1 to 16 probabilities of the pooled quantiles; ``tail``: the two
        probabilities of the tail ESS; ``scores``: also return the rank-score chains ``z`` and ``z_folded``. Returns a
        :class:`ChainRank`; padding and columns with a non-finite entry are NaN / -1."""
        chain = np.asarray(chain, np.float64)
        if chain.ndim == 2:
            chain = chain[:, None, :]
        if chain.ndim != 3:
            raise ValueError("chain must be [rows, n_chains, ld]")
        chain = np.ascontiguousarray(chain)
        rows, n, ld = chain.shape
        s2 = None
        if s2chain is not None:
            s2 = np.ascontiguousarray(np.asarray(s2chain, np.float64).reshape(rows, n))
        npr = None
        if npar is not None:
            npr = np.ascontiguousarray(np.broadcast_to(np.asarray(npar, np.int32), (n,)))
        grp, ng = rhat_groups(group, n, npr)
        ck = ChainRank.empty(ng, ld, probs, tail, max_lag, (rows, n, s2 is not None) if scores else None)
        opt, out = ck.options(), ck.to_c()
        self._check(self._lib.tci_chainrank(self._h, C.byref(opt), _lib.ptr(chain, _lib._dp), _lib.ptr(s2, _lib._dp),
                                            rows, n, ld, _lib.ptr(npr, _lib._i32p), _lib.ptr(grp, _lib._i32p), ng,
                                            C.byref(out)))
        return ck.taken(out)

    def chainlp(self, chain: np.ndarray, s2chain: np.ndarray, cell_id: Sequence[int], prior_mu: np.ndarray,
                prior_sig: np.ndarray) -> ChainLp:
        """The sum-of-squares trace of chains held on the host (mcmcstat's ``sschain``, ``mcmcrun``'s fourth output),
        with the prior, deviance and log-posterior of every row and, per chain, the best sample (a posterior-mode
        estimate) and DIC, on the device (``tci_chainlp``; the definition is in ``include/tci.h``). ``chain``
        ``[rows, n_chains, ld]`` (or ``[rows, ld]``: one chain), ``s2chain`` ``[rows, n_chains]``, ``cell_id`` one
        cell per chain, ``prior_mu`` / ``prior_sig`` ``[n_chains, ld]`` as for ``dram_run``. Returns a
        :class:`ChainLp`; a chain with a non-finite ss, prior or deviance anywhere has NaN reductions and
        ``best_row = -1``."""
        chain = np.asarray(chain, np.float64)
        if chain.ndim == 2:
            chain = chain[:, None, :]
        if chain.ndim != 3:
            raise ValueError("chain must be [rows, n_chains, ld]")
        chain = np.ascontiguousarray(chain)
        rows, n, ld = chain.shape
        s2 = np.ascontiguousarray(np.asarray(s2chain, np.float64).reshape(rows, n))
        cid = np.ascontiguousarray(np.atleast_1d(cell_id), np.int32)
        if cid.shape != (n,):
            raise ValueError("cell_id must have one entry per chain")
        mu = np.ascontiguousarray(np.asarray(prior_mu, np.float64).reshape(n, ld))
        sig = np.ascontiguousarray(np.asarray(prior_sig, np.float64).reshape(n, ld))
        cl = ChainLp.empty(rows, n, ld)
        opt, out = cl.options(), cl.to_c()
        self._check(self._lib.tci_chainlp(self._h, C.byref(opt), _lib.ptr(chain, _lib._dp), _lib.ptr(s2, _lib._dp), rows,
                                          n, ld, _lib.ptr(cid, _lib._i32p), _lib.ptr(mu, _lib._dp),
                                          _lib.ptr(sig, _lib._dp), C.byref(out)))
        cl.n_rows, cl.kernel_ms = int(out.n_rows), float(out.kernel_ms)
        return cl

    def modesearch(self, pop0: np.ndarray, cell_id: Sequence[int], lower: np.ndarray, upper: np.ndarray,
                   prior_mu: np.ndarray, prior_sig: np.ndarray, s2=None, n_gen: int = 500, F: float = 0.5,
                   CR: float = 0.9, seed: int = 0, keys=None, flags: int = 0) -> ModeSearch:
        """Differential evolution (DE/rand/1/bin) on ``f = ss / s2 + prior`` over a population per cell, on the device
        (``tci_modesearch``; the definition is in ``include/tci.h``). ``pop0`` ``[n_sel, n_pop, ld]``: the initial
        members of every selected cell, each inside ``[lower, upper]``; ``cell_id`` one cell per population; ``lower``,
        ``upper``, ``prior_mu``, ``prior_sig`` ``[n_sel, ld]`` as for ``dram_run``; ``s2`` ``[n_sel]`` or a scalar
        (default 1, the reference's ``model.sigma2``); ``keys`` ``[n_sel]``: the RNG stream key of every cell (default:
        its position). Returns a :class:`ModeSearch`."""
        pop0 = np.ascontiguousarray(pop0, np.float64)
        if pop0.ndim != 3:
            raise ValueError("pop0 must be [n_sel, n_pop, ld]")
        n, n_pop, ld = pop0.shape
        cid = np.ascontiguousarray(np.atleast_1d(cell_id), np.int32)
        if cid.shape != (n,):
            raise ValueError("cell_id must have one entry per population")
        if isinstance(n_gen, bool) or int(n_gen) != n_gen or int(n_gen) < 0:
            raise ValueError("n_gen must be an integer >= 0")
        f = lambda a: np.ascontiguousarray(np.asarray(a, np.float64).reshape(n, ld))  # noqa: E731
        lo, up, mu, sig = f(lower), f(upper), f(prior_mu), f(prior_sig)
        s2v = np.ascontiguousarray(np.broadcast_to(np.asarray(1.0 if s2 is None else s2, np.float64), (n,)))
        kv = None if keys is None else np.ascontiguousarray(keys, np.int64)
        if kv is not None and kv.shape != (n,):
            raise ValueError("keys must have one entry per population")
        ms = ModeSearch.empty(n, n_pop, ld, int(n_gen))
        opt = _lib.tci_modesearch_options(int(n_gen), float(F), float(CR), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                          _lib.ptr(kv, _lib._i64p), int(flags))
        out = ms.to_c()
        P = lambda a: _lib.ptr(a, _lib._dp)  # noqa: E731
        self._check(self._lib.tci_modesearch(self._h, C.byref(opt), P(pop0), ld, _lib.ptr(cid, _lib._i32p), n, n_pop,
                                             P(lo), P(up), P(mu), P(sig), P(s2v), C.byref(out)))
        ms.n_evals, ms.kernel_ms = int(out.n_evals), float(out.kernel_ms)
        return ms

    def demc(self, pop0: np.ndarray, cell_id: Sequence[int], lower: np.ndarray, upper: np.ndarray,
             prior_mu: np.ndarray, prior_sig: np.ndarray, jitter: np.ndarray, sigma2_0=1.0, n_gen: int = 1000,
             thin: int = 1, jump_every: int = 10, CR: float = 0.2, gamma0: float = 0.0, updatesigma: bool = True,
             seed: int = 0, keys=None, stats_from: int = 0, rhat: bool = False, ess: bool = False, max_lag: int = 0,
             log_rows: int = 0, flags: int = 0, rank=False) -> Demc:
        """Differential-evolution Markov chain (ter Braak 2006) over a population per cell, on the device
        (``tci_demc_run``; the definition is in ``include/tci.h``). ``pop0`` ``[n_sel, n_pop, ld]``: the initial members
        of every selected cell, each inside ``[lower, upper]``; ``cell_id`` one cell per population; ``lower``,
        ``upper``, ``prior_mu``, ``prior_sig`` and ``jitter`` ``[n_sel, ld]``; ``sigma2_0`` ``[n_sel]`` or a scalar;
        ``keys`` ``[n_sel]``: the RNG stream key of every cell (default: its position). ``rhat`` / ``ess``: also the
        group reductions of the kept rows of generations ``>= stats_from`` across every cell's members, taken from the
        device chain; ``rank``: ``True`` or a dict of ``probs`` / ``tail``: the rank diagnostics of :meth:`chainrank`
        over the same rows and groups too (``tci_demc_run_rank``). ``log_rows``: generations the decision logs keep.
        Returns a :class:`Demc`."""
        pop0 = np.ascontiguousarray(pop0, np.float64)
        if pop0.ndim != 3:
            raise ValueError("pop0 must be [n_sel, n_pop, ld]")
        n, n_pop, ld = pop0.shape
        cid = np.ascontiguousarray(np.atleast_1d(cell_id), np.int32)
        if cid.shape != (n,):
            raise ValueError("cell_id must have one entry per population")
        for name, v in (("n_gen", n_gen), ("thin", thin), ("log_rows", log_rows)):
            if isinstance(v, bool) or int(v) != v or int(v) < 0:
                raise ValueError(f"{name} must be an integer >= 0")
        f = lambda a: np.ascontiguousarray(np.asarray(a, np.float64).reshape(n, ld))  # noqa: E731
        lo, up, mu, sig, jit = f(lower), f(upper), f(prior_mu), f(prior_sig), f(jitter)
        s2v = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma2_0, np.float64), (n,)))
        kv = None if keys is None else np.ascontiguousarray(keys, np.int64)
        if kv is not None and kv.shape != (n,):
            raise ValueError("keys must have one entry per population")
        dm = Demc.empty(n, n_pop, ld, int(n_gen), int(thin), int(log_rows))
        opt = _lib.tci_demc_options(int(n_gen), int(thin), int(jump_every), int(stats_from), int(updatesigma), float(CR),
                                    float(gamma0), int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.ptr(kv, _lib._i64p), int(flags))
        out = dm.to_c()
        cr = ChainRhat.empty(n, ld) if rhat else None
        ce = ChainEss.empty(n, ld, max_lag) if ess else None
        ropt, rout = (cr.options(), cr.to_c()) if cr is not None else (None, None)
        eopt, eout = (ce.options(), ce.to_c()) if ce is not None else (None, None)
        R = lambda x: None if x is None else C.byref(x)  # noqa: E731
        P = lambda a: _lib.ptr(a, _lib._dp)  # noqa: E731
        ck = None
        if rank is not None and rank is not False:
            ck = ChainRank.empty(n, ld, max_lag=max_lag, **({} if rank is True else dict(rank)))
        args = (self._h, C.byref(opt), P(pop0), ld, _lib.ptr(cid, _lib._i32p), n, n_pop, P(lo), P(up), P(mu), P(sig), P(jit),
                P(s2v), C.byref(out), R(ropt), R(rout), R(eopt), R(eout))
        if ck is not None:
            kopt, kout = ck.options(), ck.to_c()
            self._check(self._lib.tci_demc_run_rank(*args, C.byref(kopt), C.byref(kout)))
            dm.rank = ck.taken(kout)
        else:
            self._check(self._lib.tci_demc_run(*args))
        dm.kernel_ms = float(out.kernel_ms)
        if cr is not None:
            cr.n_rows, cr.kernel_ms = int(rout.n_rows), float(rout.kernel_ms)
        if ce is not None:
            ce.n_rows, ce.kernel_ms = int(eout.n_rows), float(eout.kernel_ms)
        dm.rhat, dm.ess = cr, ce
        return dm

    def demczs(self, pop0: np.ndarray, z0: np.ndarray, cell_id: Sequence[int], lower: np.ndarray, upper: np.ndarray,
               prior_mu: np.ndarray, prior_sig: np.ndarray, jitter: np.ndarray, sigma2_0=1.0, n_gen: int = 1000,
               thin: int = 1, jump_every: int = 10, CR: float = 0.2, gamma0: float = 0.0, updatesigma: bool = True,
               seed: int = 0, keys=None, stats_from: int = 0, append_every: int = 10, p_snooker: float = 0.1,
               rhat: bool = False, ess: bool = False, max_lag: int = 0, log_rows: int = 0, flags: int = 0, rank=False,
               archive: bool = False, bounds: str = "reject", census: bool = False) -> DemcZs:
        """DE-MC(zs) (ter Braak & Vrugt 2008) on the device (``tci_demczs_run``; the definition is in ``include/tci.h``):
        ``n_pop`` chains per cell whose proposals come from an archive of past states, with snooker moves. ``pop0``
        ``[n_sel, n_pop, ld]``: the chains' starts; ``z0`` ``[n_sel, m0, ld]``: the starting archive of every cell,
        ``m0 >= 3`` rows inside ``[lower, upper]``; ``append_every``: the chains' states join the archive after every
        such generation; ``p_snooker``: the share of snooker moves; ``archive``: also return the final archive.
        ``bounds``: ``'reject'`` (a proposal with a coordinate outside the box is rejected unevaluated) or ``'reflect'``
        (the oriented reflection of ``tci_demczs_run_bounds``); ``census``: also count, per chain and coordinate, how
        often the coordinate crossed and how often it left below or above its bound. With the defaults the call is
        ``tci_demczs_run`` as before. Everything else is :meth:`demc`'s. Returns a :class:`DemcZs`."""
        if bounds not in ("reject", "reflect"):
            raise ValueError("bounds must be 'reject' or 'reflect'")
        if not isinstance(census, (bool, np.bool_)):
            raise ValueError("census must be True or False")
        pop0 = np.ascontiguousarray(pop0, np.float64)
        z0 = np.ascontiguousarray(z0, np.float64)
        if pop0.ndim != 3:
            raise ValueError("pop0 must be [n_sel, n_pop, ld]")
        n, n_pop, ld = pop0.shape
        if z0.ndim != 3 or z0.shape[0] != n or z0.shape[2] != ld:
            raise ValueError("z0 must be [n_sel, m0, ld]")
        m0 = z0.shape[1]
        cid = np.ascontiguousarray(np.atleast_1d(cell_id), np.int32)
        if cid.shape != (n,):
            raise ValueError("cell_id must have one entry per population")
        for name, v in (("n_gen", n_gen), ("thin", thin), ("log_rows", log_rows)):
            if isinstance(v, bool) or int(v) != v or int(v) < 0:
                raise ValueError(f"{name} must be an integer >= 0")
        if isinstance(append_every, bool) or int(append_every) != append_every:
            raise ValueError("append_every must be an integer")
        f = lambda a: np.ascontiguousarray(np.asarray(a, np.float64).reshape(n, ld))  # noqa: E731
        lo, up, mu, sig, jit = f(lower), f(upper), f(prior_mu), f(prior_sig), f(jitter)
        s2v = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma2_0, np.float64), (n,)))
        kv = None if keys is None else np.ascontiguousarray(keys, np.int64)
        if kv is not None and kv.shape != (n,):
            raise ValueError("keys must have one entry per population")
        # an archive the library will refuse (its own message) is not allocated here
        ok = int(append_every) >= 1 and m0 + n_pop * (int(n_gen) // max(int(append_every), 1)) < 2 ** 24
        dm = DemcZs.empty_zs(n, n_pop, ld, int(n_gen), int(thin), int(log_rows), m0, int(append_every), archive and ok)
        opt = _lib.tci_demczs_options(int(n_gen), int(thin), int(jump_every), int(stats_from), int(updatesigma), float(CR),
                                      float(gamma0), int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.ptr(kv, _lib._i64p), int(flags),
                                      int(append_every), float(p_snooker))
        out = dm.to_c()
        cr = ChainRhat.empty(n, ld) if rhat else None
        ce = ChainEss.empty(n, ld, max_lag) if ess else None
        ropt, rout = (cr.options(), cr.to_c()) if cr is not None else (None, None)
        eopt, eout = (ce.options(), ce.to_c()) if ce is not None else (None, None)
        R = lambda x: None if x is None else C.byref(x)  # noqa: E731
        P = lambda a: _lib.ptr(a, _lib._dp)  # noqa: E731
        ck = None
        if rank is not None and rank is not False:
            ck = ChainRank.empty(n, ld, max_lag=max_lag, **({} if rank is True else dict(rank)))
        args = (self._h, C.byref(opt), P(pop0), P(z0), ld, _lib.ptr(cid, _lib._i32p), n, n_pop, m0, P(lo), P(up), P(mu),
                P(sig), P(jit), P(s2v), C.byref(out), R(ropt), R(rout), R(eopt), R(eout))
        if bounds != "reject" or census:
            bopt = _lib.tci_bounds_options(_lib.TCI_BOUNDS_REFLECT if bounds == "reflect" else _lib.TCI_BOUNDS_REJECT,
                                           int(census), 0)
            bout = dm.with_bounds(bounds, census)
            kopt, kout = (ck.options(), ck.to_c()) if ck is not None else (None, None)
            self._check(self._lib.tci_demczs_run_bounds(*args, R(kopt), R(kout), C.byref(bopt), C.byref(bout)))
            if ck is not None:
                dm.rank = ck.taken(kout)
        elif ck is not None:
            kopt, kout = ck.options(), ck.to_c()
            self._check(self._lib.tci_demczs_run_rank(*args, C.byref(kopt), C.byref(kout)))
            dm.rank = ck.taken(kout)
        else:
            self._check(self._lib.tci_demczs_run(*args))
        dm.kernel_ms, dm.n_archive = float(out.kernel_ms), int(out.n_archive)
        if cr is not None:
            cr.n_rows, cr.kernel_ms = int(rout.n_rows), float(rout.kernel_ms)
        if ce is not None:
            ce.n_rows, ce.kernel_ms = int(eout.n_rows), float(eout.kernel_ms)
        dm.rhat, dm.ess = cr, ce
        return dm

    # -- evaluation (device buffers, asynchronous) --------------------------
    def ss_batch_device(self, theta, cell_id, out, active=None, stream=None) -> None:
        """Launch on device tensors already resident in HBM (torch tensors or raw pointers):
        ``theta`` (B, ld) float64, ``cell_id`` (B,) int32, ``out`` (B,) float64, optional
        ``active`` (B,) uint8. ``stream``: a torch stream / raw hipStream_t (None or 0 = the
        HIP default stream). Nothing is synchronised."""
        def addr(x):
            if x is None:
                return None
            return x.data_ptr() if hasattr(x, "data_ptr") else int(x)

        if hasattr(theta, "shape"):
            B, ld = int(theta.shape[0]), int(theta.shape[1])
            self._check_device_args(theta, cell_id, out, active, B)
        else:
            raise ValueError("theta must be a 2-D device tensor")
        st = getattr(stream, "cuda_stream", stream)
        self._check(self._lib.tci_ss_batch_async(self._h, addr(theta), ld, addr(cell_id), addr(active), B, addr(out),
                                                 st))

    @staticmethod
    def _check_device_args(theta, cell_id, out, active, B):
        import torch

        if theta.dtype != torch.float64 or not theta.is_contiguous() or not theta.is_cuda:
            raise ValueError("theta must be a contiguous float64 device tensor")
        if cell_id.dtype != torch.int32 or cell_id.numel() != B or not cell_id.is_cuda:
            raise ValueError("cell_id must be an int32 device tensor with one entry per row")
        if out.dtype != torch.float64 or out.numel() < B or not out.is_cuda:
            raise ValueError("out must be a float64 device tensor with >= B entries")
        if active is not None and (active.dtype != torch.uint8 or active.numel() != B or not active.is_cuda):
            raise ValueError("active must be a uint8 device tensor with one entry per row")


def version() -> str:
    return _lib.load().tci_version().decode()
