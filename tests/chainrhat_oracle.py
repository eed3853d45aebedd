"""Restatement of the group reduction of include/tci.h (tci_chainrhat: classic and split R-hat, pooled mean and
standard deviation of every group of chains) in numpy, in FP64 (`table(..., dtype=np.float64)`, the formulas as the
device rounds them, with the sums in a choice of orders) and in numpy.longdouble (the reference the bound is taken
against). Test infrastructure: the device never runs this.

The error bound (u = 2^-53, X = max|x| over the group's column, a sequence has L rows, a statistic m sequences)
----------------------------------------------------------------------------------------------------------------
mu_j    A compensated sum (Neumaier; compensated partial sums combined by a compensated sum are one) is within
        2 u |S| + O(L u^2) sum|x| of S; total() and the division add one rounding each, so with L u < 2^-20
          |mu^_j - mu_j| <= d := 4 u X.
        A constant sequence's mean is exact.
s2_j    Taken about mu^_j instead of mu_j the centred sum grows by exactly L (mu^_j - mu_j)^2 <= L d^2 (second
        order). Each term (x - mu^_j)^2 carries 3 roundings, the sum of L non-negative terms at most L - 1 more in
        any order, the division one: relative (L + 3) u.
W       The sum of m non-negative s2_j and a division: relative (L + m + 3) u, and absolute 2 d^2 from the means.
T       Let e_j = mu^_j - mu_j (|e_j| <= d). A common error of mubar shifts every difference alike and enters
        sum_j (mu^_j - mubar^)^2 at second order only (m times its square, and the plain sum of the m means is within
        m u X of its value): the first-order change is 2 sum_j (mu_j - mubar)(e_j - ebar), by Cauchy-Schwarz at most
        2 sqrt((m - 1) T) sqrt(m) d. Divided by m - 1:  |dT| <= 2 sqrt(2) sqrt(T) d  +  2 (1 + m^2 / 16) d^2, on top
        of the roundings of the differences, squares, sum and division: relative (m + 4) u.
rhat    rhat^2 = a + T / W with a = (L - 1) / L (one rounding), T / W relative (L + 2 m + 8) u, the sum and the
        square root one rounding each, and the reference's own rounding to FP64 one more. Since a <= rhat^2 and
        T / W <= rhat^2 and d rhat = d(rhat^2) / (2 rhat):
          relative      ((L + 2 m + 9) / 2 + 2) u rhat              <= (L + 2 m + 16) u rhat
          cancellation  2 sqrt(2) sqrt(T) d / (2 W rhat)            <= 8 u X sqrt(T) / (W rhat)
          second order  (2 (1 + m^2 / 16) d^2 / W) / (2 rhat) + (T / W) (2 d^2 / W) / (2 rhat)
                                                                    <= (m^2 + 32) (u X)^2 (rhat + 1 / rhat) / W
        The cancellation term is the one that matters for a column far from 0 next to its spread (a hierarchical
        fit's v: X = 5, sqrt(W) = 1e-6); for a column centred within a few spreads of 0 it is a few u.
pooled_mean  within d + m u X = (m + 4) u X.
pooled_std   V = ((n - 1) sum s2_j + n sum (mu_j - mubar)^2) / (M n): the relative roundings sum to at most
        (n + m + 8) u V, the means change n sum(..) / (M n) by at most 2 d sqrt(V); std = sqrt(V) halves the relative
        part and adds a rounding: within (n + m + 10) u std + 8 u X (the second term covers d and the second order).
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53           # unit roundoff of FP64
ORDERS = ("forward", "reversed", "pairwise")
OUTPUTS = ("rhat", "rhat_split", "pooled_mean", "pooled_std")


def _neumaier(rows, dtype):
    """(s, c) of Neumaier's sum over the arrays `rows` yields."""
    s = c = None
    for r in rows:
        if s is None:
            s, c = np.zeros(r.shape, dtype), np.zeros(r.shape, dtype)
        t = s + r
        c = c + np.where(np.abs(s) >= np.abs(r), (s - t) + r, (r - t) + s)
        s = t
    return s, c


def csum(x, order="forward", block=32):
    """The compensated sum of x [L, ...] along axis 0 in x's dtype. 'pairwise': blocks of `block` rows, the blocks'
    (s, c) pairs combined as the device combines its partial sums (s by a compensated add, c by a plain one)."""
    if order == "forward":
        s, c = _neumaier(iter(x), x.dtype)
    elif order == "reversed":
        s, c = _neumaier(iter(x[::-1]), x.dtype)
    else:
        parts = [_neumaier(iter(x[i:i + block]), x.dtype) for i in range(0, len(x), block)]
        s, c = _neumaier((p[0] for p in parts), x.dtype)
        for p in parts:
            c = c + p[1]
    return s + c


def _plain(x, order):
    if order == "pairwise":
        return np.sum(x, axis=0)
    acc = np.zeros(x.shape[1:], x.dtype)
    for r in (x if order == "forward" else x[::-1]):
        acc = acc + r
    return acc


def seq_moments(x, order="forward"):
    """mu and s2 of the sequences x [L, ...] (x's dtype): compensated mean, a constant sequence's mean its value,
    two-pass centred s2 = sum (x - mu)^2 / (L - 1); L < 2: s2 is NaN, L == 0: mu too."""
    L = x.shape[0]
    nan = np.full(x.shape[1:], np.nan, x.dtype)
    if L == 0:
        return nan, nan
    const = np.all(x == x[0], axis=0)
    mu = np.where(const, x[0], csum(x, order) / x.dtype.type(L))
    if L < 2:
        return mu, nan
    d = x - mu
    return mu, _plain(d * d, order) / x.dtype.type(L - 1)


def psrf(mu, s2, L):
    """The between/within combination of the m sequences mu, s2 [m, ...] of length L, in sequence order:
    rhat, sum s2, mubar, sum (mu - mubar)^2, W, T."""
    m, tp = mu.shape[0], mu.dtype.type
    sv, sm = np.zeros(mu.shape[1:], mu.dtype), np.zeros(mu.shape[1:], mu.dtype)
    for k in range(m):
        sv = sv + s2[k]
        sm = sm + mu[k]
    mubar = np.where(np.all(mu == mu[0], axis=0), mu[0], sm / tp(m))
    dev = np.zeros(mu.shape[1:], mu.dtype)
    for k in range(m):
        d = mu[k] - mubar
        dev = dev + d * d
    with np.errstate(divide="ignore", invalid="ignore"):
        W = sv / tp(m)
        T = dev / tp(m - 1) if m >= 2 else np.full_like(dev, np.nan)
        rhat = np.sqrt(tp(L - 1) / tp(L) + T / W) if (m >= 2 and L >= 2) else np.full_like(dev, np.nan)
    return rhat, sv, mubar, dev, W, T


def table(chain, s2chain=None, npar=None, group=None, dtype=np.float64, order="forward"):
    """The four outputs of tci_chainrhat for chain [rows, n_chains, ld] as arrays [n_groups, ld + 1] (s2 is the last
    column; NaN without s2chain) in `dtype`, and what the bound needs: W, T, W_split, T_split, X (max|x| of the
    group's column) [n_groups, ld + 1] and M [n_groups]."""
    chain = np.asarray(chain, np.float64)
    n, nc, ld = chain.shape
    npar = np.full(nc, ld) if npar is None else np.broadcast_to(np.asarray(npar), (nc,))
    group = np.zeros(nc, np.int64) if group is None else np.asarray(group)
    ng = max(int(group.max()) + 1, 1)
    x = np.full((n, nc, ld + 1), np.nan)
    x[:, :, :ld] = chain
    if s2chain is not None:
        x[:, :, ld] = np.asarray(s2chain, np.float64).reshape(n, nc)
    live = np.arange(ld + 1)[None, :] < npar[:, None]
    live[:, ld] = s2chain is not None
    bad = ~np.all(np.isfinite(x), axis=0) | ~live
    xs = np.where(bad[None], 0.0, x).astype(dtype)
    h = n // 2
    with np.errstate(invalid="ignore", divide="ignore"):
        mom = [seq_moments(xs, order), seq_moments(xs[:h], order), seq_moments(xs[n - h:], order)]
    out = {k: np.full((ng, ld + 1), np.nan, dtype) for k in OUTPUTS + ("W", "T", "W_split", "T_split")}
    out["X"] = np.zeros((ng, ld + 1))
    out["M"] = np.zeros(ng, np.int64)
    tp = np.dtype(dtype).type
    for g in range(ng):
        cs = np.nonzero(group == g)[0]
        M = out["M"][g] = len(cs)
        if M == 0:
            continue
        assert len(set(int(npar[c]) for c in cs)) == 1, "mixed npar in a group"
        ok = ~np.any(bad[cs], axis=0)
        rh, sv, mubar, dev, W, T = psrf(mom[0][0][cs], mom[0][1][cs], n)
        mu2 = np.stack([mom[1 + k % 2][0][cs[k // 2]] for k in range(2 * M)])
        s22 = np.stack([mom[1 + k % 2][1][cs[k // 2]] for k in range(2 * M)])
        rh2, _, _, _, W2, T2 = psrf(mu2, s22, h)
        with np.errstate(invalid="ignore"):
            std = np.sqrt((tp(n - 1) * sv + tp(n) * dev) / (tp(M) * tp(n)))
        for k, v in (("rhat", rh), ("rhat_split", rh2), ("pooled_mean", mubar), ("pooled_std", std), ("W", W),
                     ("T", T), ("W_split", W2), ("T_split", T2)):
            out[k][g] = np.where(ok, v, np.nan)
        out["X"][g] = np.max(np.abs(np.where(bad[None, cs], 0.0, x[:, cs])), axis=(0, 1))
    return out


def bounds(ref, n):
    """The bounds of the module docstring for every output, from the longdouble table `ref`: [n_groups, ld + 1]."""
    f = lambda a: np.asarray(a, np.float64)  # noqa: E731
    X, M = ref["X"], ref["M"][:, None].astype(np.float64)

    def rb(rhat, T, W, L, m):
        rhat, T, W = f(rhat), f(T), f(W)
        with np.errstate(invalid="ignore", divide="ignore"):
            return ((L + 2 * m + 16) * U * rhat + 8 * U * X * np.sqrt(T) / (W * rhat)
                    + (m * m + 32) * (U * X) ** 2 * (rhat + 1 / rhat) / W)

    return {"rhat": rb(ref["rhat"], ref["T"], ref["W"], n, M),
            "rhat_split": rb(ref["rhat_split"], ref["T_split"], ref["W_split"], n // 2, 2 * M),
            "pooled_mean": (M + 4) * U * X,
            "pooled_std": (n + M + 10) * U * f(ref["pooled_std"]) + 8 * U * X}


def joined(cr):
    """A ChainRhat as the table's arrays [n_groups, ld + 1]."""
    return {k: np.concatenate([getattr(cr, k), getattr(cr, "s2_" + k)[:, None]], axis=1) for k in OUTPUTS}


def check(got, ref, n, where=""):
    """`got` (arrays [n_groups, ld + 1] per output) against the longdouble table `ref`: NaN and +Inf where and only
    where the reference has them, every finite value within its bound. Returns the largest error in units of its
    bound and the largest bound of each output."""
    bnd = bounds(ref, n)
    worst, widest = {}, {}
    for k in OUTPUTS:
        g, w = np.asarray(got[k], np.float64), np.asarray(ref[k]).astype(np.float64)
        assert g.shape == w.shape, (where, k, g.shape, w.shape)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (where, k, "NaN pattern")
        assert np.array_equal(np.isinf(g), np.isinf(w)), (where, k, "Inf pattern")
        ok = np.isfinite(w)
        err = np.abs(g[ok].astype(LD) - np.asarray(ref[k])[ok]).astype(np.float64)
        tol = bnd[k][ok]
        assert np.all(np.isfinite(tol)), (where, k, "bound not finite")
        ratio = err / np.maximum(tol, 1e-300)
        assert np.all(err <= tol), (where, k, float(np.max(ratio)))
        worst[k] = float(np.max(ratio, initial=0.0))
        widest[k] = float(np.max(tol, initial=0.0))
    return worst, widest


# ---- fixtures shared by the host and the device tests ----------------------------------------------------------

NS = (2, 3, 4, 31, 32, 33, 255, 256, 257, 513, 1000)   # both sides of the 8 / 32-row step and the 256-row segment
LDS = (1, 7, 63, 64, 65, 136)
MS = (1, 2, 3, 4, 7)


def walk_chains(seed, rows, n_chains, ld, npar):
    """Random-walk chains [rows, n_chains, ld] and s2 [rows, n_chains]: per column a seeded mean within a few units
    of 0 and a step scale between 1e-2 and 1e2 (no column sits far from 0 next to its spread: that is the offset
    fixture's). Padding columns (j >= npar) hold values that are not 0: padding has to be masked, not inferred."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-2.0, 2.0, (n_chains, ld))
    mean = rng.standard_normal((n_chains, ld))
    x = mean[None] + scale[None] * np.cumsum(rng.standard_normal((rows, n_chains, ld)), axis=0)
    for c, P in enumerate(npar):
        x[:, c, int(P):] = 7.0 + rng.standard_normal((rows, ld - int(P)))
    s2 = 1.0 + rng.gamma(4.0, 0.25, (rows, n_chains))
    return np.ascontiguousarray(x), np.ascontiguousarray(s2)


def shape_case(i):
    """Case i of the shape sweep: n = NS[i], ld and three group sizes cycling through LDS and MS, ragged npar across
    the groups, two chains in no group; even i: the chains shuffled (groups interleave) and an s2 chain; odd i: the
    groups in descending id order and no s2 chain."""
    n, ld = NS[i], LDS[i % len(LDS)]
    sizes = [MS[(i + k) % len(MS)] for k in (0, 2, 3)]
    np_g = [ld, max(1, ld - 3), max(1, (ld + 1) // 2)]
    rng = np.random.default_rng(1000 + i)
    ids = np.concatenate([np.full(m, g) for g, m in enumerate(sizes)] + [np.full(2, -1)])
    ids = rng.permutation(ids) if i % 2 == 0 else np.sort(ids)[::-1]
    npar = np.array([np_g[g] if g >= 0 else ld for g in ids], np.int32)
    chain, s2 = walk_chains(2000 + i, n, len(ids), ld, npar)
    return {"name": f"n{n}_ld{ld}_M{'-'.join(map(str, sizes))}", "chain": chain, "s2": s2 if i % 2 == 0 else None,
            "npar": npar, "group": np.ascontiguousarray(ids, np.int32), "n": n}


def special_case():
    """M = 3 chains of 300 rows, 8 columns: 0 a walk; 1 the same constant in every chain (W = T = 0: NaN); 2 constant
    in chain 0 only; 3 a different constant per chain (W = 0, T > 0: +Inf); 4 a NaN and 5 a +Inf in one chain; 6
    identical in the three chains (exactly sqrt((L - 1) / L)); 7 a walk."""
    chain, s2 = walk_chains(77, 300, 3, 8, [8, 8, 8])
    chain[:, :, 1] = 2.5
    chain[:, 0, 2] = -1.25
    chain[:, :, 3] = np.array([1.0, 2.0, 4.0])[None]
    chain[17, 1, 4] = np.nan
    chain[299, 2, 5] = np.inf
    chain[:, :, 6] = chain[:, :1, 6]
    return {"name": "special", "chain": chain, "s2": s2, "npar": np.full(3, 8, np.int32),
            "group": np.zeros(3, np.int32), "n": 300}


def offset_case():
    """The hierarchical v: M = 4 chains of 1000 rows near 5 with spread 1e-6 (column 0; column 1 is a walk)."""
    rng = np.random.default_rng(5)
    chain, s2 = walk_chains(78, 1000, 4, 2, [2, 2, 2, 2])
    chain[:, :, 0] = 5.0 + 1e-6 * rng.standard_normal((1000, 4))
    return {"name": "offset", "chain": chain, "s2": s2, "npar": np.full(4, 2, np.int32),
            "group": np.zeros(4, np.int32), "n": 1000}


def all_cases():
    return [shape_case(i) for i in range(len(NS))] + [special_case(), offset_case()]
