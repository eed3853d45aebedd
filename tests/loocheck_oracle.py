"""Numpy restatement of PSIS-LOO and the stacking weights (tci_loocheck, include/tci.h), for the tests. Host only.

ll_s and lr_s use +, -, x and / on host values, so they are float64 with the device's bits in both paths, and so are
the tail's membership, its order and cut. From exp onwards there are two paths over them:

  exact=False  float64, every operation and every sum in the contract's order; differs from the device by the roundings
               of exp, log, log1p and expm1 (numpy's here, the device library's there).
  exact=True   the same statements in np.longdouble (64-bit mantissa). The largest difference between the two paths on
               the test inputs, times 8, is the tests' tolerance (profiles/loocheck/tolerance.json).
"""
import math

import numpy as np

import fitcheck_oracle as FO

POINTWISE = ("elpd_loo_i", "lppd_i", "p_loo_i", "khat_i")
SIGN = np.uint64(0x8000000000000000)


def tail_count(S):
    """M = min(floor(S / 5), ceil(3 sqrt(S))) and G = 30 + floor(sqrt(M))."""
    if not 32 <= S <= 4096:
        raise ValueError("S must be in [32, 4096]")
    M = min(S // 5, int(math.ceil(3.0 * math.sqrt(float(S)))))
    return M, 30 + int(math.floor(math.sqrt(float(M))))


def default_threshold(S):
    return min(1.0 - 1.0 / math.log10(float(S)), 0.7)


def to_key(x):
    """The order-preserving map of doubles to uint64 (-0 < +0, NaN above +Inf)."""
    x = np.ascontiguousarray(x, np.float64)
    u = x.view(np.uint64).copy()
    u[np.isnan(x)] = np.uint64(0x7FF8000000000000)
    return np.where((u & SIGN) != 0, ~u, u | SIGN)


def log_lik(sim, y, s2):
    """ll [S, N] float64, the device's bits, and the scored mask [N]."""
    sim = np.asarray(sim, np.float64)
    y = np.asarray(y, np.float64)
    sd, lg, _ = FO.host_rows(s2)
    with np.errstate(all="ignore"):
        r = y[None, :] - sim
        z = r / sd[:, None]
        ll = -0.5 * (lg[:, None] + z * z)
    return ll, np.isfinite(y) & np.all(np.isfinite(sim), axis=0)


def select_tail(ll):
    """lr [S, N], the sample index of tail_1 .. tail_M per point [M, N], and cut [N]: all exact."""
    S = ll.shape[0]
    M, _ = tail_count(S)
    with np.errstate(all="ignore"):
        lr = -ll
        lr = lr - np.max(lr, axis=0)[None, :]
    order = np.argsort(to_key(lr), axis=0, kind="stable")  # ties: ascending s
    return lr, order[S - M:], np.take_along_axis(lr, order[S - M - 1:S - M], axis=0)[0]


def psis(ll, exact=False):
    """The pointwise values of every column of ll [S, N] (no scored mask applied) and the smoothed lw [S, N]."""
    T = np.longdouble if exact else np.float64
    S, N = ll.shape
    M, G = tail_count(S)
    lr, tail_idx, cut = select_tail(ll)
    tail = np.take_along_axis(lr, tail_idx, axis=0)

    def total(a):
        tot = np.zeros(a.shape[1:], T)
        for s0 in range(0, a.shape[0], FO.SEG):
            part = np.zeros(a.shape[1:], T)
            for s in range(s0, min(s0 + FO.SEG, a.shape[0])):
                part = part + a[s]
            tot = tot + part
        return tot

    with np.errstate(all="ignore"):
        ec = np.exp(cut.astype(T))
        x = np.exp(tail.astype(T)) - ec[None, :]
        xM, x1, xq = x[M - 1], x[0], x[(M + 2) // 4 - 1]
        degenerate = ~(xM > 0) | ~np.isfinite(xM) | (x1 < 0)
        dM = T(M)
        c = T(1.0) - np.sqrt(T(G) / (np.arange(1, G + 1).astype(T) - T(0.5)))
        bg = (T(1.0) / xM)[None, :] + c[:, None] / (T(3.0) * xq)[None, :]      # [G, N]
        acc = np.zeros((G, N), T)
        for j in range(M):
            acc = acc + np.log1p(-bg * x[j][None, :])
        kg = acc / dM
        L = dM * ((np.log(-bg / kg) + (-kg)) - T(1.0))
        den = np.zeros((G, N), T)
        for h in range(G):
            den = den + np.exp(L[h][None, :] - L)
        wg = T(1.0) / den
        b = np.zeros(N, T)
        for g in range(G):
            b = b + bg[g] * wg[g]
        acc = np.zeros(N, T)
        for j in range(M):
            acc = acc + np.log1p(-b * x[j])
        k = acc / dM
        sigma = -k / b
        khat = (k * dM + T(5.0)) / T(M + 10)
        degenerate = degenerate | ~np.isfinite(khat) | ~np.isfinite(sigma)
        p = (np.arange(1, M + 1).astype(T) - T(0.5)) / dM
        q = sigma[None, :] * np.expm1(-khat[None, :] * np.log1p(-p)[:, None]) / khat[None, :]
        sm = np.minimum(np.log(q + ec[None, :]), T(0.0))
        new_tail = np.where(degenerate[None, :], tail.astype(T), sm)
        khat = np.where(degenerate, T(np.inf), khat)
        lw = lr.astype(T)
        np.put_along_axis(lw, tail_idx, new_tail, axis=0)
        a = lw + ll.astype(T)
        mA, mB = np.max(a, axis=0), np.max(lw, axis=0)
        elpd = (mA + np.log(total(np.exp(a - mA[None, :])))) - (mB + np.log(total(np.exp(lw - mB[None, :]))))
        m = np.max(ll, axis=0).astype(T)
        logS = np.log(T(S)) if exact else T(math.log(float(S)))
        lppd = (m + np.log(total(np.exp(ll.astype(T) - m[None, :])))) - logS
    return {"elpd_loo_i": elpd, "lppd_i": lppd, "p_loo_i": lppd - elpd, "khat_i": khat}, lw


def pointwise(sim, y, s2, exact=False):
    """One dye of one chain: sim [S, N] simulated rows, y [N] data, s2 [S]: the four pointwise vectors [N], NaN at
    unscored points."""
    ll, scored = log_lik(sim, y, s2)
    out, _ = psis(ll, exact)
    return {k: np.where(scored, v, np.nan) for k, v in out.items()}


def per_chain(pt, threshold):
    """The per-chain values from pt[name] = [2, N] (dye 0, then dye 1, ascending j, scored points, sums from 0.0)."""
    n_obs, n_bad = 0, 0
    T = np.asarray(pt["elpd_loo_i"]).dtype.type
    elpd, ploo, lppd, kmax = T(0.0), T(0.0), T(0.0), -np.inf
    for d in range(2):
        for j in range(np.shape(pt["khat_i"])[1]):
            kh = pt["khat_i"][d][j]
            if np.isnan(kh):
                continue
            n_obs += 1
            elpd = elpd + pt["elpd_loo_i"][d][j]
            lppd = lppd + pt["lppd_i"][d][j]
            ploo = ploo + pt["p_loo_i"][d][j]
            kmax = max(kmax, float(kh))
            n_bad += bool(kh > threshold)
    if n_obs == 0:
        nan = float("nan")
        return {"n_obs": 0, "elpd_loo": nan, "p_loo": nan, "lppd": nan, "khat_max": nan, "n_khat_bad": 0}
    return {"n_obs": n_obs, "elpd_loo": elpd, "p_loo": ploo, "lppd": lppd, "khat_max": kmax, "n_khat_bad": n_bad}


def chain(sim0, sim1, y0, y1, s2, threshold=None, exact=False):
    """A whole chain: the pointwise vectors as [2, N] and the per-chain values."""
    a, b = pointwise(sim0, y0, s2, exact), pointwise(sim1, y1, s2, exact)
    out = {k: np.stack([a[k], b[k]]) for k in a}
    out.update(per_chain(out, default_threshold(len(s2)) if threshold is None else threshold))
    return out


def stack(e, max_iter=5000, tol=1e-12, trace=False):
    """The stacking weights of one group: e [C, len], the chains' pointwise elpd_loo flattened (dye 0, then dye 1).
    Returns weights [C], elpd_stack, n_points, n_iter (and with trace=True the objective before every iteration and at
    the end)."""
    e = np.asarray(e)
    T = e.dtype.type
    C = e.shape[0]
    e = e[:, np.all(np.isfinite(e), axis=0)]
    n = e.shape[1]
    if C == 0 or n == 0:
        return (np.full(C, np.nan), float("nan"), n, 0) + (([],) if trace else ())
    m = np.max(e, axis=0)
    E = np.exp(e - m[None, :])
    w = np.full(C, T(1.0) / T(C), dtype=e.dtype)

    def objective(w):
        tot = T(0.0)
        for i in range(n):
            den = T(0.0)
            for c in range(C):
                den = den + w[c] * E[c, i]
            tot = tot + (m[i] + np.log(den))
        return tot

    objs, n_iter = [], 0
    for it in range(1, (max_iter if C > 1 else 0) + 1):
        if trace:
            objs.append(objective(w))
        a = w[:, None] * E
        den = np.zeros(n, e.dtype)
        for c in range(C):
            den = den + a[c]
        r = a / den[None, :]
        num = np.zeros(C, e.dtype)
        for i in range(n):
            num = num + r[:, i]
        wn = num / T(n)
        delta = np.max(np.abs(wn - w))
        w, n_iter = wn, it
        if delta <= tol:
            break
    es = objective(w)
    if trace:
        objs.append(es)
    return (w, es, n, n_iter) + ((objs,) if trace else ())
