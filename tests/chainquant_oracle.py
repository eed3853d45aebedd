"""Restatement of the posterior quantiles of include/tci.h (tci_chainquant) in numpy: the 64-bit keys, np.sort
of the keys, the keys mapped back, then plims' interpolation in two roundings, with the non-finite and padding
rules of the header. The device is compared with this bit for bit. Test infrastructure: the device never runs
this.

Against numpy.quantile(method='linear') the results may differ in their last bits, because the two round
differently. With u = 2^-53, M = max(|y[lo]|, |y[lo+1]|), d = y[lo+1] - y[lo] (|d| <= 2 M) and the same
f = h - floor(h) in both (h = (n-1) p is one rounded product, its fraction is exact):
  here    y[lo] + f d              rounds d, f d and the sum: three roundings of quantities no larger than 2 M.
          The first two errors are at most f u |d| each, the last at most u M:  (4 f + 1) u M.
  numpy   the same form for f < 0.5:                                           (4 f + 1) u M,
          y[lo+1] - (1 - f) d for f >= 0.5, which also rounds 1 - f:           (6 (1 - f) + 1) u M.
The sum of the two is (8 f + 2) u M < 6 u M below f = 0.5 and (8 - 2 f) u M <= 7 u M from there on, so
|here - numpy| <= 8 * 2^-53 * M (BOUND_VS_NUMPY) always holds."""
import numpy as np

SIGN = np.uint64(1 << 63)
BOUND_VS_NUMPY = 8 * 2.0 ** -53


def to_key(x):
    """The total order of the header: all bits inverted for a negative x (sign bit set), else the sign bit set."""
    u = np.ascontiguousarray(x, np.float64).view(np.uint64)
    return np.where(u & SIGN != 0, ~u, u | SIGN)


def from_key(k):
    k = np.asarray(k, np.uint64)
    return np.where(k & SIGN != 0, k ^ SIGN, ~k).view(np.float64)


def sort_column(x):
    """x [n] sorted ascending by key (-0 before +0)."""
    return from_key(np.sort(to_key(x)))


def rank_of(n, p):
    """lo and f of prob p over n rows: h = (n-1) p, lo = floor(h), f = h - lo."""
    h = np.float64(n - 1) * np.float64(p)
    lo = np.floor(h)
    return int(lo), np.float64(h - lo)


def quantiles(x, probs):
    """[nq] quantiles of the column x [n] (float64); all NaN when x holds a non-finite value."""
    x = np.asarray(x, np.float64)
    n = len(x)
    out = np.full(len(probs), np.nan)
    if not np.all(np.isfinite(x)):
        return out
    y = sort_column(x)
    for q, p in enumerate(probs):
        lo, f = rank_of(n, p)
        if lo + 1 < n:
            with np.errstate(over="ignore", invalid="ignore"):
                d = np.float64(y[lo + 1] - y[lo])        # rounded
                out[q] = y[lo] + np.float64(f * d)      # the product rounded, then the sum: never fused
        else:
            out[q] = y[n - 1]
    return out


def table(chain, s2chain=None, npar=None, probs=(0.025, 0.5, 0.975)):
    """The outputs of tci_chainquant for chain [rows, n_chains, ld]: q [n_chains, nq, ld] and s2_q [n_chains, nq];
    padding, and s2_q without an s2 chain, are NaN."""
    chain = np.asarray(chain, np.float64)
    rows, n, ld = chain.shape
    npar = np.full(n, ld) if npar is None else np.broadcast_to(np.asarray(npar), (n,))
    probs = np.atleast_1d(np.asarray(probs, np.float64))
    q = np.full((n, len(probs), ld), np.nan)
    s2_q = np.full((n, len(probs)), np.nan)
    for c in range(n):
        for j in range(int(npar[c])):
            q[c, :, j] = quantiles(chain[:, c, j], probs)
        if s2chain is not None:
            s2_q[c] = quantiles(np.asarray(s2chain, np.float64).reshape(rows, n)[:, c], probs)
    return {"q": q, "s2_q": s2_q}


def same(got, want):
    """Bitwise equality of a ChainQuant with a table."""
    return got.q.tobytes() == want["q"].tobytes() and got.s2_q.tobytes() == want["s2_q"].tobytes()


def repeated_rows(seed, rows, n_chains, ld):
    """A chain that rejects: every random row repeated a random 1 to 30 times, cut to `rows` rows."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, n_chains, ld)) * 10.0 ** rng.uniform(-3, 3, (1, n_chains, ld))
    reps = rng.integers(1, 31, rows)
    return np.ascontiguousarray(np.repeat(x, reps, axis=0)[:rows])
