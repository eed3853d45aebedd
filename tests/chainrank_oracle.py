"""numpy restatement of tci_chainrank (include/tci.h): the pooled order on the 64-bit keys, the pooled quantiles by
plims, the rank scores through statistics.NormalDist().inv_cdf, and the split statistics of the transformed chains
through chainrhat_oracle / chainess_oracle.

Exact parts. q, q_tail and every z whose p lies in the central branch of AS241 (|p - 0.5| <= 0.425: a rational
function, no transcendental) are the device's bit for bit; so are R2 and p everywhere (integers, one correctly rounded
division).

The tail-branch bound Z_TAIL_ULP. There z = -+ num(s) / den(s), s = r - 1.6 or r - 5, r = sqrt(-log(t)), t = min(p,
1 - p) <= 0.075. The device and the library agree on t bit for bit and differ in log alone. With u = 2^-53:
  log    the device math library states a maximum error of 1 ulp for FP64 log, glibc's is below 1 ulp: the two values
         of -log(t) differ by at most 2 ulp, 4 u relative.
  sqrt   correctly rounded on both sides; the square root halves a relative difference (2 u) and each side rounds once
         (u each): the two r differ by at most 4 u relative.
  z(r)   z as a function of r is the normal quantile of exp(-r^2) up to AS241's error of 1e-16: dz/dr = 2 r t /
         phi(z), and (dz/dr) (r / z) falls from 1.9 at t = 0.075 (r = 1.609, z = -1.44) towards 1 as t -> 0; at most 2.
         A relative difference of 4 u in r moves z by at most 8 u relative. The subtraction r - 1.6 or r - 5 is exact
         for r within a factor 2 of the constant (Sterbenz) and rounds once otherwise (at most 2 u in s, s >= 1.6: less
         than 2 u more in z).
  Horner every coefficient is positive and s >= 0: no cancellation, so 7 multiplications and 7 additions leave each
         polynomial within 14 u relative, the quotient within 14 + 14 + 1 = 29 u of num / den at the s it was given; two
         evaluations at their two s: 58 u.
Sum: 8 + 2 + 58 = 68 u relative, and a relative difference of k u is at most k ulp of z. Z_TAIL_ULP = 72 leaves the
second-order terms room. The test prints the largest difference it sees.
"""
import statistics

import numpy as np

import chainess_oracle as E
import chainquant_oracle as Q
import chainrhat_oracle as R

Z_TAIL_ULP = 72
_INV = statistics.NormalDist().inv_cdf


def rank2(x):
    """R2 = 2 lt + eq + 1 of every entry of the finite vector x in its own pooled key order (int64)."""
    k = Q.to_key(x)
    y = np.sort(k)
    lt = np.searchsorted(y, k, side="left").astype(np.int64)
    ub = np.searchsorted(y, k, side="right").astype(np.int64)
    return lt + ub + 1


def rank_p(r2, N):
    return (r2.astype(np.float64) - 0.75) / (np.float64(2 * N) + 0.5)


def central(p):
    return np.abs(p - 0.5) <= 0.425


def scores(x):
    """z and p of every entry of the finite vector x."""
    r2 = rank2(x)
    p = rank_p(r2, len(x))
    uniq, inv = np.unique(p, return_inverse=True)
    z = np.array([_INV(float(v)) for v in uniq])[inv]
    return z, p


def ulp_diff(a, b):
    """|a - b| in units of the spacing at b, elementwise (0 where the bits agree)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b) / np.spacing(np.abs(b))
    return np.where(a.view(np.uint64) == b.view(np.uint64), 0.0, d)


def table(chain, s2chain=None, npar=None, group=None, probs=(0.025, 0.5, 0.975), tail=(0.05, 0.95), max_lag=0,
          stats=True):
    """The outputs of tci_chainrank for chain [rows, n_chains, ld]: per-group arrays with s2 as the last column
    ([n_groups, nq, ld + 1] for q, [n_groups, 2, ld + 1] for q_tail, [n_groups, ld + 1] else), the chains z, z_folded,
    i_lo, i_hi and p, p_folded [rows, n_chains, ld + 1]. stats=False: the quantiles and chains alone."""
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
    out = {"q": np.full((ng, len(probs), ld + 1), np.nan), "q_tail": np.full((ng, 2, ld + 1), np.nan)}
    for k in ("z", "z_folded", "i_lo", "i_hi", "p", "p_folded"):
        out[k] = np.full((n, nc, ld + 1), np.nan)
    for g in range(ng):
        cs = np.nonzero(group == g)[0]
        if len(cs) == 0:
            continue
        for j in range(ld + 1):
            if not live[cs[0], j]:
                continue
            col = x[:, cs, j].T.reshape(-1)  # chains ascending, rows [0, n) of each
            if not np.all(np.isfinite(col)):
                continue
            qq = Q.quantiles(col, list(probs) + [0.5] + list(tail))
            out["q"][g, :, j] = qq[:len(probs)]
            out["q_tail"][g, :, j] = qq[len(probs) + 1:]
            z, p = scores(col)
            zf, pf = scores(np.abs(col - qq[len(probs)]))
            back = lambda v: v.reshape(len(cs), n).T  # noqa: E731
            out["z"][:, cs, j], out["p"][:, cs, j] = back(z), back(p)
            out["z_folded"][:, cs, j], out["p_folded"][:, cs, j] = back(zf), back(pf)
            out["i_lo"][:, cs, j] = back((col <= qq[len(probs) + 1]).astype(np.float64))
            out["i_hi"][:, cs, j] = back((col <= qq[len(probs) + 2]).astype(np.float64))
    if not stats:
        return out
    full = np.full(nc, ld)  # the transformed chains carry NaN where the chain had padding: the oracles skip NaN columns

    def split_stats(key, ess=True):
        t = out[key]
        c, s2 = np.ascontiguousarray(t[:, :, :ld]), (t[:, :, ld] if s2chain is not None else None)
        rh = R.table(c, s2, full, group)["rhat_split"]
        if not ess:
            return rh, None
        return rh, E.table(c, s2, full, group, max_lag=max_lag)

    with np.errstate(invalid="ignore"):
        out["rhat_bulk"], eb = split_stats("z")
        out["rhat_folded"], _ = split_stats("z_folded", ess=False)
        _, el = split_stats("i_lo")
        _, eh = split_stats("i_hi")
        out["rhat_rank"] = np.where(np.isnan(out["rhat_bulk"]) | np.isnan(out["rhat_folded"]), np.nan,
                                    np.maximum(out["rhat_bulk"], out["rhat_folded"]))
        out["ess_bulk"], out["tau_bulk"], out["window_bulk"] = eb["ess_split"], eb["tau_split"], eb["window_split"]
        out["ess_tail_lo"], out["window_tail_lo"] = el["ess_split"], el["window_split"]
        out["ess_tail_hi"], out["window_tail_hi"] = eh["ess_split"], eh["window_split"]
        out["ess_tail"] = np.where(np.isnan(out["ess_tail_lo"]) | np.isnan(out["ess_tail_hi"]), np.nan,
                                   np.minimum(out["ess_tail_lo"], out["ess_tail_hi"]))
    # a padding column or one with a non-finite entry: the transformed chains are NaN there, so the oracles above gave
    # NaN / -1 already, which is the definition
    return out


def joined(ck, name):
    """Output `name` of a ChainRank with its s2 twin as the last column."""
    a, b = getattr(ck, name), getattr(ck, "s2_" + name)
    return np.concatenate([a, b[..., None]], axis=-1)


def joined_chain(z, s2_z):
    """A rank-score chain [rows, n_chains, ld] with its s2 twin (None: NaN) as column ld."""
    last = np.full(z.shape[:2], np.nan) if s2_z is None else s2_z
    return np.concatenate([z, last[..., None]], axis=-1)
