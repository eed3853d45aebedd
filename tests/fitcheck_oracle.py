"""Numpy restatement of the posterior predictive fit checks (tci_fitcheck, include/tci.h), for the tests. Host only.

Two paths over the same simulated rows:

  exact=False  float64, every operation and every sum in the contract's order (segments of 64 samples, ascending
               inside a segment from 0.0, the partials ascending from 0.0). resid, zbar and z2 use +, -, x and / only,
               so they carry the device's bits; lppd, p_waic and pit differ from the device by the roundings of exp,
               log and erfc (numpy's and scipy's here, the device library's there).
  exact=True   np.longdouble (64-bit mantissa) for every operation, for exp and log and for the sums, and
               scipy.special.erfc at the float64 nearest to its argument: the "formulas evaluated without rounding" the
               bound is stated against, on the same float64 f_s, sd_s and lg_s. Its own error (2^-64 relative per
               operation; erfc's argument rounded to float64, at most 0.25 u in pit, and scipy's erfc, about 1 ulp) is
               inside the slack the bound's constants leave.

bounds() is the error bound of the header (DESIGN.md section 7h derives it):

  u = 2^-53, Z2 = max_s z_s^2, L = max_s |lg_s|, g = min(S, 64) + ceil(S / 64), K_exp = K_log = 3, K_erfc = 16 ulp
  E = u (4 Z2 + L)
  lppd    1.01 u (4 Z2 + L + 2 K_exp + g + (2 K_log + 4) log S + 2 |lppd|)
  A = (L + Z2) / 2;  D = 2 E + (g + 3) u A
  p_waic  1.01 (2 D sqrt(S p_waic / (S - 1)) + S D^2 / (S - 1) + (g + 4) u p_waic)
  pit     1.01 u (2 K_erfc + g + 4)
"""
import math

import numpy as np
from scipy.special import erfc

U = 2.0 ** -53
K_EXP, K_LOG, K_ERFC = 3.0, 3.0, 16.0  # ulp, OpenCL's double-precision limits (1 ulp = 2 u)
SEG = 64
POINTWISE = ("lppd_i", "p_waic_i", "pit", "resid", "zbar", "z2")
INV_SQRT2 = 0.7071067811865476
TWO_PI = 6.283185307179586


def host_rows(s2):
    """sd_s, lg_s and logS as the host computes them (the C library's sqrt and log)."""
    s2 = np.asarray(s2, np.float64)
    sd = np.array([math.sqrt(v) for v in s2])
    lg = np.array([math.log(TWO_PI * v) for v in s2])
    return sd, lg, math.log(float(len(s2)))


def seg_sum(x):
    """SUM_s over axis 0 in the contract's order; x: [S, ...] float64."""
    total = np.zeros(x.shape[1:])
    for s0 in range(0, x.shape[0], SEG):
        part = np.zeros(x.shape[1:])
        for s in range(s0, min(s0 + SEG, x.shape[0])):
            part = part + x[s]
        total = total + part
    return total


def pointwise(sim, y, s2, exact=False):
    """One dye of one cell: sim [S, N] simulated rows, y [N] data, s2 [S]. Returns the six pointwise vectors [N] (NaN at
    unscored points) and 'Z2' = max_s z_s^2 per point; with exact=True as np.longdouble."""
    sim = np.asarray(sim, np.float64)
    y = np.asarray(y, np.float64)
    S, N = sim.shape
    sd, lg, logS = host_rows(s2)
    scored = np.isfinite(y) & np.all(np.isfinite(sim), axis=0)
    T = np.longdouble if exact else np.float64
    total = (lambda a: np.sum(a, axis=0, dtype=np.longdouble)) if exact else seg_sum
    with np.errstate(all="ignore"):
        r = y.astype(T)[None, :] - sim.astype(T)
        z = r / sd.astype(T)[:, None]
        zz = z * z
        ll = T(-0.5) * (lg.astype(T)[:, None] + zz)
        m = np.max(ll, axis=0)
        if exact:
            logS = np.log(np.longdouble(S))
        lppd = (m + np.log(total(np.exp(ll - m[None, :])))) - logS
        lbar = total(ll) / T(S)
        d = ll - lbar[None, :]
        p_waic = total(d * d) / T(S - 1)
        phi = T(0.5) * erfc((-z * T(INV_SQRT2)).astype(np.float64)).astype(T)
        out = {"lppd_i": lppd, "p_waic_i": p_waic, "pit": total(phi) / T(S), "resid": total(r) / T(S),
               "zbar": total(z) / T(S), "z2": total(zz) / T(S)}
        out = {k: np.where(scored, v, T(np.nan)) for k, v in out.items()}
        out["Z2"] = np.where(scored, np.max(zz, axis=0).astype(np.float64), np.nan)
    return out


def per_cell(pt, levels):
    """The per-cell values from the pointwise vectors pt[name] = [2, N] (dye 0, then dye 1, ascending j, scored
    points only, sums from 0.0). A point is scored where pit is not NaN."""
    levels = np.asarray(levels, np.float64)
    n_obs, lppd, pw, z2 = 0, 0.0, 0.0, 0.0
    inside = np.zeros(len(levels), np.int64)
    dw = np.full(2, np.nan)
    with np.errstate(all="ignore"):
        for d in range(2):
            pit, zbar = np.asarray(pt["pit"][d], np.float64), np.asarray(pt["zbar"][d], np.float64)
            num, den, prev = np.float64(0.0), np.float64(0.0), False
            for j in range(len(pit)):
                sc = not np.isnan(pit[j])
                if sc:
                    n_obs += 1
                    lppd = lppd + np.float64(pt["lppd_i"][d][j])
                    pw = pw + np.float64(pt["p_waic_i"][d][j])
                    z2 = z2 + np.float64(pt["z2"][d][j])
                    for i, lv in enumerate(levels):
                        lo = (1.0 - lv) / 2.0
                        hi = 1.0 - lo
                        inside[i] += bool(lo <= pit[j] <= hi)
                    if prev:
                        dz = zbar[j] - zbar[j - 1]
                        num = num + dz * dz
                    den = den + zbar[j] * zbar[j]
                prev = sc
            dw[d] = num / den
    if n_obs == 0:
        nan = float("nan")
        return {"n_obs": 0, "lppd": nan, "p_waic": nan, "elpd_waic": nan, "chi2": nan,
                "coverage": np.full(len(levels), np.nan), "dw": np.full(2, np.nan)}
    return {"n_obs": n_obs, "lppd": float(lppd), "p_waic": float(pw), "elpd_waic": float(lppd - pw),
            "chi2": float(z2 / np.float64(n_obs)), "coverage": inside / np.float64(n_obs), "dw": dw}


def cell(sim0, sim1, y0, y1, s2, levels=(0.5, 0.95), exact=False):
    """A whole cell: sim0/sim1 [S, N] rows of MS2 / PP7, y0/y1 [N]. Returns the pointwise vectors as [2, N], 'Z2'
    [2, N] and the per-cell values."""
    a, b = pointwise(sim0, y0, s2, exact), pointwise(sim1, y1, s2, exact)
    out = {k: np.stack([a[k], b[k]]) for k in a}
    out.update(per_cell(out, levels))
    return out


def bounds(S, Z2, L, lppd, p_waic):
    """The header's bounds of |lppd - exact|, |p_waic - exact| and |pit - exact| at points with the given Z2, lppd and
    p_waic (arrays), for S samples with L = max_s |lg_s|."""
    Z2, lppd, p_waic = (np.asarray(a, np.float64) for a in (Z2, lppd, p_waic))
    g = min(S, SEG) + -(-S // SEG)
    E = U * (4.0 * Z2 + L)
    b_lppd = 1.01 * U * (4.0 * Z2 + L + 2 * K_EXP + g + (2 * K_LOG + 4) * math.log(S) + 2.0 * np.abs(lppd))
    A = (L + Z2) / 2.0
    D = 2.0 * E + (g + 3) * U * A
    with np.errstate(all="ignore"):
        b_pw = 1.01 * (2.0 * D * np.sqrt(S * p_waic / (S - 1.0)) + S * D * D / (S - 1.0) + (g + 4) * U * p_waic) \
            if S > 1 else np.full(Z2.shape, np.nan)
    b_pit = np.full(Z2.shape, 1.01 * U * (2 * K_ERFC + g + 4))
    return {"lppd_i": b_lppd, "p_waic_i": b_pw, "pit": b_pit}


def cell_bounds(ref, s2):
    """bounds() for a cell() result `ref` (either path) and its s2."""
    _, lg, _ = host_rows(s2)
    return bounds(len(lg), ref["Z2"], float(np.max(np.abs(lg))), np.asarray(ref["lppd_i"], np.float64),
                  np.asarray(ref["p_waic_i"], np.float64))
