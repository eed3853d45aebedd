"""Restatement of the posterior moments of include/tci.h (tci_chaincov) in numpy.longdouble: two-pass,
centred, with the clamping, diagonal, NaN and padding rules of the header. Returns float64. Test
infrastructure: the device never runs this."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53           # unit roundoff of FP64


def moments(x):
    """mean [P], cov [P, P], corr [P, P] (float64) of the rows of x [n, P], n >= 2."""
    x = np.asarray(x, np.float64)
    n, P = x.shape
    finite = np.all(np.isfinite(x), axis=0)
    xl = np.where(finite[None, :], x, 0.0).astype(LD)
    # pass 1. The sum is compensated (Neumaier, in longdouble): a chain column whose mean is small next to
    # its values has a condition number of 1e3 and more, and numpy's plain longdouble sum then carries an
    # error of its own of a few 2^-53 of the mean, more than the bound the device is held to
    s, comp = np.zeros(P, LD), np.zeros(P, LD)
    for row in xl:
        t = s + row
        comp += np.where(np.abs(s) >= np.abs(row), (s - t) + row, (row - t) + s)
        s = t
    m = (s + comp) / LD(n)
    y = xl - m[None, :]                              # pass 2, centred
    cov = (y.T @ y) / LD(n - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        sd = np.sqrt(np.diagonal(cov))
        corr = cov / (sd[:, None] * sd[None, :])     # a constant column: 0/0 = NaN in its row and column
    corr = np.clip(corr, LD(-1), LD(1))              # keeps NaN
    d = np.diagonal(cov)
    idx = np.arange(P)
    corr[idx, idx] = np.where(np.isfinite(d) & (d > 0), LD(1), LD(np.nan))
    mean, cov, corr = m.astype(np.float64), cov.astype(np.float64), corr.astype(np.float64)
    bad = ~finite                                    # a non-finite entry: the mean, the row and the column
    mean[bad] = np.nan
    for a in (cov, corr):
        a[bad, :] = np.nan
        a[:, bad] = np.nan
    return mean, cov, corr


def table(chain, npar=None):
    """The three outputs of tci_chaincov for chain [rows, n_chains, ld]: padding is NaN."""
    chain = np.asarray(chain, np.float64)
    rows, n, ld = chain.shape
    npar = np.full(n, ld) if npar is None else np.broadcast_to(np.asarray(npar), (n,))
    mean = np.full((n, ld), np.nan)
    cov = np.full((n, ld, ld), np.nan)
    corr = np.full((n, ld, ld), np.nan)
    for c in range(n):
        P = int(npar[c])
        if P > 0:
            mean[c, :P], cov[c, :P, :P], corr[c, :P, :P] = moments(chain[:, c, :P])
    return {"mean": mean, "cov": cov, "corr": corr}


def walk_chain(seed, rows, n_chains, ld, npar=None):
    """Random-walk chains [rows, n_chains, ld]: per column a seeded mean and a step scale between 1e-6 and
    1e2. Column 0 of every chain is near-constant, 5 + 1e-6 noise (v of a hierarchical fit); column 2 is
    -2 x column 1 plus a little noise (a correlation next to -1). Padding columns (j >= npar) hold values
    that are not 0: padding has to be masked, not inferred."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-6.0, 2.0, (n_chains, ld))
    mean = 10.0 * rng.standard_normal((n_chains, ld))
    x = mean[None] + scale[None] * np.cumsum(rng.standard_normal((rows, n_chains, ld)), axis=0)
    x[:, :, 0] = 5.0 + 1e-6 * rng.standard_normal((rows, n_chains))
    if ld >= 3:
        x[:, :, 2] = -2.0 * x[:, :, 1] + 1e-3 * scale[None, :, 1] * rng.standard_normal((rows, n_chains))
    if npar is not None:
        for c, P in enumerate(np.broadcast_to(np.asarray(npar), (n_chains,))):
            x[:, c, int(P):] = 7.0 + rng.standard_normal((rows, ld - int(P)))
    return np.ascontiguousarray(x)


def check(got, want, n, where=""):
    """The bounds of the issue, elementwise. cov: |dev - ref| <= (n + 8) 2^-52 sqrt(ref_ii ref_jj), the
    dot-product error bound (n products and sums at unit roundoff 2^-53, the centring and the division on
    top) with Cauchy-Schwarz on the centred columns; corr: (n + 16) 2^-52 absolute (the same bound on the
    numerator and half of it on either variance); mean: 4 x 2^-53 relative (the compensated sum is exact
    to one rounding, the division and the reference's own rounding to FP64 add one each). NaN where and
    only where the reference has NaN. Returns the largest error of each in units of its bound."""
    worst = {}
    for k in ("mean", "cov", "corr"):
        g, w = np.asarray(getattr(got, k)), want[k]
        assert g.shape == w.shape, (where, k)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (where, k, "NaN pattern")
    ok = ~np.isnan(want["mean"])
    err = np.abs(got.mean[ok] - want["mean"][ok])
    tol = 4 * U * np.abs(want["mean"][ok])
    assert np.all(err <= tol), (where, "mean", float(np.max(err / np.maximum(tol, 1e-300))))
    worst["mean"] = float(np.max(err / np.maximum(tol, 1e-300), initial=0.0))
    d = np.diagonal(want["cov"], axis1=1, axis2=2)
    with np.errstate(invalid="ignore"):
        scale = np.sqrt(d[:, :, None] * d[:, None, :])
    ok = ~np.isnan(want["cov"])
    err = np.abs(got.cov[ok] - want["cov"][ok])
    tol = (n + 8) * 2 * U * scale[ok]
    assert np.all(err <= tol), (where, "cov", float(np.max(err / np.maximum(tol, 1e-300))))
    worst["cov"] = float(np.max(err / np.maximum(tol, 1e-300), initial=0.0))
    ok = ~np.isnan(want["corr"])
    err = np.abs(got.corr[ok] - want["corr"][ok])
    tol = (n + 16) * 2 * U
    assert np.all(err <= tol), (where, "corr", float(np.max(err) / tol))
    worst["corr"] = float(np.max(err, initial=0.0) / tol)
    return worst
