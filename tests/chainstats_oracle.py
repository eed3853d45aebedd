"""numpy restatement of the chain diagnostics defined in include/tci.h (the tests' oracle):
batch-means Monte-Carlo error, Sokal's integrated autocorrelation time (FFT form for the circular
autocovariance, as mcmcstat's iact; a direct lag form to check it against) and the batch-means Geweke
test. Shared by test_chainstats_host.py, test_chainstats_gpu.py and test_chainstats_mex.py."""
import math

import numpy as np

PHIS = (0.0, 0.5, 0.9, 0.97)
RTOL_TAU = 1e-9      # tau: relative
RTOL = 1e-10         # mcerr: relative; z and p: relative to max(1, |value|)


def bm_s(x):
    """Batch-means s: b = max(10, n // 20), nb = n // b batches from row 0, centred on the mean of
    ALL rows; NaN when there are fewer than two batches."""
    x = np.asarray(x, np.float64)
    n = len(x)
    b = max(10, n // 20)
    nb = n // b
    if nb < 2:
        return math.nan
    y = x[:nb * b].reshape(nb, b).mean(axis=1)
    return math.sqrt(b * float(((y - x.mean()) ** 2).sum()) / (nb - 1))


def mcerr(x):
    n = len(x)
    return bm_s(x) / math.sqrt(n) if n >= 20 else math.nan


def acov_fft(x):
    """c(k) = sum_t y[t] y[(t + k) mod n], y = x - mean(x), for k = 0 .. n-1, through the FFT."""
    y = np.asarray(x, np.float64) - np.mean(x)
    f = np.fft.fft(y)
    return np.fft.ifft(f * np.conj(f)).real


def acov_direct(x):
    y = np.asarray(x, np.float64) - np.mean(x)
    return np.array([float(np.dot(y, np.roll(y, -k))) for k in range(len(y))])


def sokal(c, max_lag=0):
    """(tau, window, margin) from the autocovariances c: S = -1/3; S += c(i-1)/c(0) - 1/6 for i = 1, 2, ..
    until S < 0. margin: the least |S| over every step up to and including the crossing."""
    n = len(c)
    L = n if max_lag == 0 else min(int(max_lag), n)
    if c[0] == 0:
        return 0.0, 0, math.inf
    S, margin = -1.0 / 3.0, math.inf
    for i in range(1, L + 1):
        S += c[i - 1] / c[0] - 1.0 / 6.0
        margin = min(margin, abs(S))
        if S < 0:
            return 2.0 * (S + (i - 1) / 6.0), i, margin
    return math.inf, L, margin


def geweke(x):
    x = np.asarray(x, np.float64)
    n = len(x)
    na, nb = n // 10, n // 2
    if na < 20 or nb < 20:
        return math.nan, math.nan
    a, b = x[:na], x[n - nb:]
    with np.errstate(divide="ignore", invalid="ignore"):
        z = float((a.mean() - b.mean()) / np.sqrt(np.float64(bm_s(a) ** 2 / na + bm_s(b) ** 2 / nb)))
    return z, (math.erfc(abs(z) / math.sqrt(2.0)) if z == z else math.nan)


def column(x, max_lag=0, direct=False):
    """Every statistic of one column; a non-finite entry makes all of them NaN (window -1)."""
    x = np.asarray(x, np.float64)
    if not np.all(np.isfinite(x)):
        return dict(mcerr=math.nan, tau=math.nan, tau_window=-1, geweke_z=math.nan, geweke_p=math.nan, margin=math.inf)
    if np.all(x == x[0]):   # centred on its value exactly: c(0) == 0, s == 0, Geweke 0/0
        z = math.nan
        return dict(mcerr=0.0 if len(x) >= 20 else math.nan, tau=0.0, tau_window=0, geweke_z=z, geweke_p=z,
                    margin=math.inf)
    tau, w, margin = sokal(acov_direct(x) if direct else acov_fft(x), max_lag)
    z, p = geweke(x)
    return dict(mcerr=mcerr(x), tau=tau, tau_window=w, geweke_z=z, geweke_p=p, margin=margin)


def table(chain, s2=None, npar=None, max_lag=0):
    """The oracle over a whole chain [rows][n_chains][ld] (+ s2 [rows][n_chains]): dict of arrays shaped
    like the library's outputs, padding NaN / -1, and 'margin' = the least Sokal margin over every column."""
    rows, n, ld = chain.shape
    npar = np.full(n, ld) if npar is None else np.asarray(npar)
    out = {k: np.full((n, ld), np.nan) for k in ("mcerr", "tau", "geweke_z", "geweke_p")}
    out["tau_window"] = np.full((n, ld), -1, np.int32)
    for k in ("mcerr", "tau", "geweke_z", "geweke_p"):
        out["s2_" + k] = np.full(n, np.nan)
    out["s2_tau_window"] = np.full(n, -1, np.int32)
    margin = math.inf
    for c in range(n):
        for j in range(int(npar[c])):
            r = column(chain[:, c, j], max_lag)
            margin = min(margin, r.pop("margin"))
            for k, v in r.items():
                out[k][c, j] = v
        if s2 is not None:
            r = column(s2[:, c], max_lag)
            margin = min(margin, r.pop("margin"))
            for k, v in r.items():
                out["s2_" + k][c] = v
    out["margin"] = margin
    return out


def ar1_columns(rng, rows, ncols):
    """AR(1) columns 3 + 2 x with phi cycling through PHIS, stationary start."""
    phi = np.array([PHIS[k % len(PHIS)] for k in range(ncols)])
    e = rng.standard_normal((rows, ncols))
    x = np.empty((rows, ncols))
    x[0] = e[0] / np.sqrt(1.0 - phi ** 2)
    for t in range(1, rows):
        x[t] = phi * x[t - 1] + e[t]
    return 3.0 + 2.0 * x


def rel_err(got, want, floor_one=False):
    """Largest |got - want| / |want| (or / max(1, |want|)); NaN and Inf must sit in the same places."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN pattern differs"
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), "Inf pattern differs"
    if not fin.any():
        return 0.0
    den = np.maximum(1.0, np.abs(want[fin])) if floor_one else np.abs(want[fin])
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(got[fin] == want[fin], 0.0, np.abs(got[fin] - want[fin]) / den)
    return float(e.max())


def check(st, want, label=""):
    """Assert a ChainStats (or anything with its attributes) against table()'s result at the tolerances
    the diagnostics are held to; returns the errors seen."""
    errs = {}
    for pre in ("", "s2_"):
        assert np.array_equal(getattr(st, pre + "tau_window"), want[pre + "tau_window"]), label + pre + "tau_window"
        errs[pre + "tau"] = rel_err(getattr(st, pre + "tau"), want[pre + "tau"])
        errs[pre + "mcerr"] = rel_err(getattr(st, pre + "mcerr"), want[pre + "mcerr"])
        errs[pre + "geweke_z"] = rel_err(getattr(st, pre + "geweke_z"), want[pre + "geweke_z"], floor_one=True)
        errs[pre + "geweke_p"] = rel_err(getattr(st, pre + "geweke_p"), want[pre + "geweke_p"], floor_one=True)
    print(label, {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v <= (RTOL_TAU if k.endswith("tau") else RTOL), (label, k, v)
    return errs
