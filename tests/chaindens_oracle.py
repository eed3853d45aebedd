"""Restatement of the marginal densities and histograms of include/tci.h (tci_chaindens) in numpy: the key-order
extremes, the compensated mean, the two-pass sd, the quartiles of tests/chainquant_oracle.py, the bandwidth, the
grid in its pinned roundings, the Gaussian kernel sum and the equal-width bins, with the constant, non-finite and
padding rules of the header. Test infrastructure: the device never runs this.

range, the grid and counts are pinned IEEE operations on exact order statistics: the device is compared with them
bit for bit. bw and dens depend on a summation order and on exp, so they carry bounds, derived here and not fitted
to any output. With u = 2^-53 and n rows:

  bw    Each centred square (x - m)^2 carries three roundings (the difference, which enters twice, and the
        product): 3 u. Any summation order of n non-negative terms adds at most (n - 1) u. The division by n - 1
        adds u, the square root halves what came before and adds u: ((n + 3) / 2 + 1) u for sd. An error dm of
        the mean m changes the sum by n dm^2, second order: the compensated mean is right to an ulp or two of |m|,
        and (ulp(m) / sd)^2 stays below u for every column whose sd exceeds 1e-8 |m|. iqr is the difference of two
        quantiles that are tci_chainquant's float64 values by definition (exact inputs, not estimates of a real
        quantile), one rounding, and iqr / 1.34 one more. The three products of the bandwidth and pow add
        5 u. In all below (n / 2 + 11) u, so
            |bw - exact| <= (n + 16) u bw                                              (BW_REL)
        holds with room for either branch of min(sd, iqr / 1.34).
  dens  The grid is exact (both sides compute the same bits). z = (g - x) / bw carries 2 u (3 u where the device
        multiplies by a rounded 1 / bw) plus the bandwidth's relative error d. The exponent a = z^2 / 2 then
        carries 2 (3 u + d) + 2 u relative, and exp turns a relative error e of a into a e^-a <= 1/e in absolute
        terms: at most (8 u + 2 d) / e < 3 u + d per term, plus one ulp for exp itself: (4 u + d) per term of a
        sum in which every term is at most 1. A sum of n non-negative terms adds at most n u of the total. The
        total, scaled by 1 / (n bw sqrt(2 pi)), never exceeds peak = 1 / (bw sqrt(2 pi)), the value n coincident
        rows give. The scale factor has three roundings and the bandwidth's d again; |d y / d ln bw| <= peak. So
            |dens - exact| <= ((4 + n + 3) u + 3 d) peak <= (4 n + 96) u peak          (DENS_ABS)
        with d <= (n + 16) u.
The restatement itself is held to the same bounds against its own formulas evaluated in numpy.longdouble
(tests/test_chaindens_host.py), so a comparison of the device with it is not a comparison with its errors."""
import math

import numpy as np

import chainquant_oracle as Q

U = 2.0 ** -53
INV_SQRT_2PI = 1.0 / math.sqrt(2.0 * math.pi)


def bw_rel(n):
    """Relative bound of bw."""
    return (n + 16) * U


def dens_abs(n, bw):
    """Absolute bound of every dens[k] of a column with bandwidth bw (array or scalar)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return (4 * n + 96) * U * INV_SQRT_2PI / np.asarray(bw, np.float64)


def grid_of(xmin, xmax, G):
    """[G] grid of the header: lo = xmin - 0.08 r, hi = xmax + 0.08 r, step = (hi - lo) / (G - 1), lo + k step;
    numpy rounds every operation once."""
    xmin, xmax = np.float64(xmin), np.float64(xmax)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.float64(xmax - xmin)
        w = np.float64(0.08 * r)
        lo, hi = np.float64(xmin - w), np.float64(xmax + w)
        step = np.float64(np.float64(hi - lo) / np.float64(G - 1))
        return lo + np.arange(G, dtype=np.float64) * step


def extremes(x):
    """(xmin, xmax) in key order: -0 below +0."""
    k = Q.to_key(x)
    return Q.from_key(k.min())[()], Q.from_key(k.max())[()]


def bins_of(x, xmin, xmax, B):
    """[B] int32 counts: row t in bin min(B - 1, floor((x_t - xmin) / r * B)); r == 0: all rows in bin 0."""
    r = np.float64(xmax - xmin)
    if not r > 0:
        out = np.zeros(B, np.int32)
        out[0] = len(x)
        return out
    b = np.floor((x - xmin) / r * np.float64(B)).astype(np.int64)
    return np.bincount(np.minimum(B - 1, b), minlength=B).astype(np.int32)


def bandwidth(x, bw_scale=1.0):
    """bw of the column x (finite, n >= 2)."""
    n = len(x)
    m = x[0] if np.all(x == x[0]) else np.float64(math.fsum(x) / n)   # a constant column: its value, sd exactly 0
    sd = np.sqrt(np.sum((x - m) ** 2) / np.float64(n - 1))
    q25, q75 = Q.quantiles(x, [0.25, 0.75])
    iqr = np.float64(q75 - q25)
    s = min(sd, iqr / 1.34) if iqr > 0 else sd
    return np.float64(np.float64(np.float64(np.float64(bw_scale) * 1.06) * s) * np.float64(n) ** -0.2)


def kde(x, g, bw):
    """[len(g)] Gaussian kernel estimate at g with bandwidth bw; all NaN for bw == 0."""
    n = len(x)
    if not bw > 0:
        return np.full(len(g), np.nan)
    out = np.empty(len(g))
    for k0 in range(0, len(g), 16):              # blocks of grid points bound the temporary
        z = (g[k0:k0 + 16, None] - x[None, :]) / bw
        out[k0:k0 + 16] = np.exp(-(z * z) / 2.0).sum(axis=1) / (n * bw) * INV_SQRT_2PI
    return out


def column(x, G=100, B=20, bw_scale=1.0):
    """The outputs of one column: range [2], bw, dens [G], counts [B], grid [G]."""
    x = np.ascontiguousarray(x, np.float64)
    if not np.all(np.isfinite(x)):
        return {"range": np.full(2, np.nan), "bw": np.nan, "dens": np.full(G, np.nan),
                "counts": np.full(B, -1, np.int32), "grid": np.full(G, np.nan)}
    xmin, xmax = extremes(x)
    bw = bandwidth(x, bw_scale)
    g = grid_of(xmin, xmax, G)
    return {"range": np.array([xmin, xmax]), "bw": bw, "dens": kde(x, g, bw), "counts": bins_of(x, xmin, xmax, B),
            "grid": g}


def column_longdouble(x, G=100, bw_scale=1.0):
    """bw and dens [G] of a finite column by the same formulas in numpy.longdouble, on the float64 grid."""
    x = np.ascontiguousarray(x, np.float64)
    n = len(x)
    L = np.longdouble
    xl = x.astype(L)
    m = xl.sum() / L(n)
    sd = np.sqrt(((xl - m) ** 2).sum() / L(n - 1))
    qs = Q.quantiles(x, [0.25, 0.75]).astype(L)   # the definition's quartiles are tci_chainquant's float64 values
    iqr = qs[1] - qs[0]
    s = min(sd, iqr / L(1.34)) if iqr > 0 else sd
    bw = L(bw_scale) * L(1.06) * s * L(n) ** (L(-1) / L(5))
    g = grid_of(*extremes(x), G).astype(L)
    if not bw > 0:
        return bw, np.full(G, np.nan, L)
    z = (g[:, None] - xl[None, :]) / bw
    dens = np.exp(-(z * z) / L(2)).sum(axis=1) / (L(n) * bw) / np.sqrt(L(2) * L(np.pi))
    return bw, dens


def table(chain, s2chain=None, npar=None, n_grid=100, n_bins=20, bw_scale=1.0):
    """The outputs of tci_chaindens for chain [rows, n_chains, ld], as a dict of the ChainDens arrays plus grid
    [n_chains, G, ld] and s2_grid [n_chains, G]; padding, and the s2 twins without an s2 chain, are NaN / -1."""
    chain = np.asarray(chain, np.float64)
    rows, n, ld = chain.shape
    npar = np.full(n, ld) if npar is None else np.broadcast_to(np.asarray(npar), (n,))
    G, B = n_grid, n_bins
    t = {"range": np.full((n, 2, ld), np.nan), "bw": np.full((n, ld), np.nan), "dens": np.full((n, G, ld), np.nan),
         "counts": np.full((n, B, ld), -1, np.int32), "grid": np.full((n, G, ld), np.nan),
         "s2_range": np.full((n, 2), np.nan), "s2_bw": np.full(n, np.nan), "s2_dens": np.full((n, G), np.nan),
         "s2_counts": np.full((n, B), -1, np.int32), "s2_grid": np.full((n, G), np.nan)}
    for c in range(n):
        for j in range(int(npar[c])):
            col = column(chain[:, c, j], G, B, bw_scale)
            for k, v in col.items():
                t[k][c, ..., j] = v
        if s2chain is not None:
            col = column(np.asarray(s2chain, np.float64).reshape(rows, n)[:, c], G, B, bw_scale)
            for k, v in col.items():
                t["s2_" + k][c] = v
    return t


def compare(got, want, n, where=""):
    """A ChainDens against a table: range, grid and counts by their bytes, bw and dens within the derived bounds,
    NaN exactly where the table has NaN. Returns the largest bw and dens errors in units of their bounds."""
    worst = [0.0, 0.0]
    for pre, grid in (("", got.grid()), ("s2_", got.s2_grid())):
        for k, g in (("range", getattr(got, pre + "range")), ("counts", getattr(got, pre + "counts")), ("grid", grid)):
            w = want[pre + k]
            assert g.shape == w.shape and g.dtype == w.dtype, (where, pre + k, g.shape, w.shape, g.dtype)
            if g.tobytes() != w.tobytes():         # equal bits, or NaN where the table has NaN
                nan = (g != g) & (w != w)
                bad = np.argwhere(~nan & ((g != w) | (np.signbit(g) != np.signbit(w))))
                assert bad.size == 0, (where, pre + k, "differs at", bad[:5].tolist())
        bw, wbw = getattr(got, pre + "bw"), want[pre + "bw"]
        assert np.array_equal(np.isnan(bw), np.isnan(wbw)), (where, pre + "bw NaN pattern")
        with np.errstate(invalid="ignore", divide="ignore"):
            e = np.abs(bw - wbw) / (bw_rel(n) * np.abs(wbw))
        e = np.where(bw == wbw, 0.0, e)
        assert not np.any(e > 1.0), (where, pre + "bw", float(np.nanmax(e)))
        worst[0] = max(worst[0], float(np.max(np.nan_to_num(e, posinf=0.0), initial=0.0)))
        d, wd = getattr(got, pre + "dens"), want[pre + "dens"]
        assert d.shape == wd.shape and np.array_equal(np.isnan(d), np.isnan(wd)), (where, pre + "dens NaN pattern")
        tol = dens_abs(n, wbw)[:, None] if pre else dens_abs(n, wbw)[:, None, :]
        with np.errstate(invalid="ignore"):
            e = np.abs(d - wd) / tol
        assert not np.any(e > 1.0), (where, pre + "dens", float(np.nanmax(e)))
        worst[1] = max(worst[1], float(np.max(np.nan_to_num(e, posinf=0.0), initial=0.0)))
    return worst
