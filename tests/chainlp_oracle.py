"""numpy restatement of tci_chainlp (include/tci.h): the prior sum in its 64-partial order, the deviance and the
log-posterior of every chain row, and the per-chain reductions in their 256-row segments. float64 throughout, every
operation rounded once in the stated order, so pri and every reduction of given traces are the device's bits. dev, lp
and d_hat go through log: `exact=True` evaluates them in long double, and bounds() restates the header's bound.
Host only: numpy."""
import numpy as np

TWO_PI = 6.283185307179586
SEG = 256       # rows per segment of every sum over rows
LANES = 64      # partial sums of the prior
K_LOG = 3       # the device log's error in ulp (1 ulp = 2 u), the figure of tci_fitcheck
U = 2.0 ** -53
LD = np.longdouble
SCALARS = ("ss_min", "ss_mean", "dev_mean", "dev_var", "lp_best", "ss_best", "s2_best", "s2_mean", "ss_hat", "d_hat",
           "p_d", "p_v", "dic")


def pri_terms(theta, mu, sig):
    """((theta_j - mu_j) / sig_j)^2 for the P entries given: a subtraction, a division, a multiplication."""
    with np.errstate(all="ignore"):
        q = (np.asarray(theta, np.float64) - mu) / sig
        return q * q


def pri(theta, mu, sig):
    """pri of rows theta [B, P] (or [P]) under mu, sig [P]: partial l adds the terms j = l, l + 64, .. ascending from
    0.0, the 64 partials are then added in ascending l from 0.0."""
    t = np.atleast_2d(pri_terms(theta, mu, sig))
    B, P = t.shape
    R = -(-P // LANES)
    # a missing term adds nothing: every term is >= +0 or NaN, and x + 0.0 is x for both
    pad = np.zeros((B, R * LANES))
    pad[:, :P] = t
    pad = pad.reshape(B, R, LANES)
    with np.errstate(all="ignore"):
        part = np.zeros((B, LANES))
        for r in range(R):
            part = part + pad[:, r]
        tot = np.zeros(B)
        for lane in range(LANES):
            tot = tot + part[:, lane]
    return tot if np.ndim(theta) > 1 else tot[0]


def pri_plain(theta, mu, sig):
    """The same terms added in plain ascending j: NOT the definition (the contrast of the host test)."""
    tot = np.float64(0.0)
    for x in pri_terms(theta, mu, sig):
        tot = tot + x
    return tot


def dev(ss, s2, nobs, exact=False):
    """ss / s2 + nobs * log(2 pi s2); exact: in long double."""
    T = LD if exact else np.float64
    ss, s2, nobs = np.asarray(ss, T), np.asarray(s2, T), np.asarray(nobs, T)
    with np.errstate(all="ignore"):
        return ss / s2 + nobs * np.log(T(TWO_PI) * s2)


def lp(dev_, pri_, exact=False):
    T = LD if exact else np.float64
    with np.errstate(all="ignore"):
        return T(-0.5) * (np.asarray(dev_, T) + np.asarray(pri_, T))


def bounds(ss, s2, nobs, dev_, lp_):
    """(E_dev, E_lp) of the header at the float64 values given."""
    ss, s2, dev_, lp_ = (np.asarray(a, np.float64) for a in (ss, s2, dev_, lp_))
    with np.errstate(all="ignore"):
        L = np.abs(np.log(TWO_PI * s2))
        e_dev = 1.01 * U * (np.abs(ss / s2) + nobs * (1.0 + (2 * K_LOG + 1) * L) + np.abs(dev_))
        return e_dev, 0.5 * e_dev + 1.01 * U * np.abs(lp_)


def seg_sum(x):
    """Sum over axis 0 of x [n, ...]: 256-row segments, ascending t from 0.0 inside, the segment sums ascending from
    0.0."""
    x = np.asarray(x, np.float64)
    tot = np.zeros(x.shape[1:])
    with np.errstate(all="ignore"):
        for r0 in range(0, len(x), SEG):
            acc = np.zeros(x.shape[1:])
            for row in x[r0:r0 + SEG]:
                acc = acc + row
            tot = tot + acc
    return tot


def col_mean(x):
    """tci_chaincov's mean of the columns of x [n, P], the same bits: Neumaier's sum in row order divided by n, a
    constant column's mean its value, NaN for a column holding a non-finite value."""
    x = np.asarray(x, np.float64)
    n, P = x.shape
    s, c = np.zeros(P), np.zeros(P)
    with np.errstate(all="ignore"):
        for row in x:
            t = s + row
            c = c + np.where(np.abs(s) >= np.abs(row), (s - t) + row, (row - t) + s)
            s = t
        m = (s + c) / np.float64(n)
    m = np.where(np.all(x == x[0], axis=0), x[0], m)
    return np.where(np.all(np.isfinite(x), axis=0), m, np.nan)


def traces(chain, s2, ss, P, nobs, mu, sig):
    """pri, dev, lp [n, C] of chain [n, C, ld] from its ss [n, C] (the likelihood kernel's); P, nobs [C]."""
    n, C, _ = chain.shape
    p = np.stack([pri(chain[:, c, :P[c]], mu[c, :P[c]], sig[c, :P[c]]) for c in range(C)], axis=1)
    d = dev(ss, s2, np.asarray(nobs, np.float64)[None, :])
    return p, d, lp(d, p)


def reduce(tr, s2, chain, P, nobs, theta_mean, s2_mean, ss_hat):
    """The per-chain reductions from the traces tr = {ss, pri, dev, lp} [n, C], s2 [n, C], chain [n, C, ld] and the
    chain's theta_mean [C, ld], s2_mean [C] and ss_hat [C] (the likelihood kernel's SS of theta_mean)."""
    n, C, ld = chain.shape
    out = {f: np.full(C, np.nan) for f in SCALARS}
    out["best_row"] = np.full(C, -1, np.int64)
    out["theta_best"] = np.full((C, ld), np.nan)
    out["theta_mean"] = np.full((C, ld), np.nan)
    with np.errstate(all="ignore"):
        for c in range(C):
            ss, pr, dv, l = (np.asarray(tr[f], np.float64)[:, c] for f in ("ss", "pri", "dev", "lp"))
            if not (np.all(np.isfinite(ss)) and np.all(np.isfinite(pr)) and np.all(np.isfinite(dv))):
                continue
            dn = np.float64(n)
            o = {"ss_min": np.min(ss), "ss_mean": seg_sum(ss) / dn, "dev_mean": seg_sum(dv) / dn}
            d = dv - o["dev_mean"]
            o["dev_var"] = seg_sum(d * d) / np.float64(n - 1)
            b = int(np.argmax(l))  # the first of the largest
            o.update(lp_best=l[b], ss_best=ss[b], s2_best=s2[b, c], s2_mean=s2_mean[c], ss_hat=ss_hat[c])
            o["d_hat"] = dev(ss_hat[c], s2_mean[c], np.float64(nobs[c]))
            o["p_d"] = o["dev_mean"] - o["d_hat"]
            o["p_v"] = 0.5 * o["dev_var"]
            o["dic"] = o["dev_mean"] + o["p_d"]
            for f in SCALARS:
                out[f][c] = o[f]
            out["best_row"][c] = b
            out["theta_best"][c, :P[c]] = chain[b, c, :P[c]]
            out["theta_mean"][c, :P[c]] = theta_mean[c, :P[c]]
    return out
