"""Restatement of the multi-chain effective sample size of include/tci.h (tci_chainess) in numpy with a dtype switch:
FP64 (`table(..., dtype=np.float64)`, the formulas as the device rounds them, the lag sums in a choice of orders) and
numpy.longdouble (the reference the bound is taken against). The lag sums are direct, no FFT. The moments (mu_j, s2_j,
W, mubar, T, pooled_std) come from chainrhat_oracle, as the device takes them from tci_chainrhat. Test infrastructure:
the device never runs this.

The error bound (u = 2^-53, X = max|x| over the group's column, a sequence has L rows, a statistic m sequences,
lambda = L / (L - 1) <= 2, s pairs are summed; chainrhat_oracle has d = 4 u X for a mean and the bounds of W and T)
----------------------------------------------------------------------------------------------------------------------
y       y^_t = fl(x_t - mu^_j) differs from y_t by at most d + u (|y_t| + d): the mean's error, common to the rows of
        a sequence, and the subtraction's rounding.
c_j(k)  sum_t (y^_t y^_{t+k} - y_t y_{t+k}) is to first order sum_t (e_t y_{t+k} + y_t e_{t+k}). With
        sum_t |y_t| <= sqrt(L sum y^2) <= L sigma_j (sigma_j^2 = s2_j) and sum_t |y_t y_{t+k}| <= sum y^2 =
        (L - 1) s2_j (Cauchy-Schwarz), it is at most 2 d L sigma_j + 2 u (L - 1) s2_j, and the second order at most
        L (d + 2 u X)^2 <= 36 L (u X)^2. The L - k products and their sum, in any order, fused or not, add at most
        (L + 1) u sum_t |y_t y_{t+k}| <= (L + 1) u (L - 1) s2_j. Divided by L (one rounding, |c_j(k) / L| <= s2_j):
          |c_j(k) / L - exact| <= 2 d sigma_j + (L + 4) u s2_j + 36 (u X)^2.
a(k)    The m quotients added (at most m roundings of a sum whose terms are at most s2_j in size) and divided by m;
        mean_j sigma_j <= sqrt(W):
          E_a = 8 u X sqrt(W) + (L + m + 6) u W + 36 (u X)^2.
W - a   W is within (L + m + 3) u W + 32 (u X)^2 (chainrhat_oracle); |W - a(k)| <= 2 W, one rounding:
          E_Wa = E_a + (L + m + 5) u W + 32 (u X)^2.
vplus   ((L - 1) / L) W carries W's error and two roundings; T is within 8 sqrt(2) u X sqrt(T) + (2 m^2 + 32) (u X)^2 +
        (m + 4) u T (chainrhat_oracle's dT with d = 4 u X); the sum one rounding; both parts are at most vplus:
          E_v = (L + 2 m + 10) u vplus + 12 u X sqrt(T) + (2 m^2 + 96) (u X)^2.
rho     r = (W - a) / vplus, |r| <= 2 W / vplus <= 2 lambda; the quotient and 1 - r one rounding each, |rho| <= 1 + 2 lambda:
          E_rho = (E_Wa + 2 lambda E_v) / vplus + (4 lambda + 1) u.
P_i     two rho and a rounding of a sum at most 2 (1 + 2 lambda):  E_P = 2 E_rho + (2 + 4 lambda) u.
tau     Q_i = min(P_i, Q_{i-1}) moves by at most E_P (min is 1-Lipschitz in the largest change of its arguments). The
        sum of s positive Q_i, sum Q = (tau + 1) / 2, adds (s - 1) u sum Q; 2 * sum is exact, -1 + . one rounding, the
        reference's own rounding to FP64 one more:
          E_tau = 2 s E_P + (s + 2) u (|tau| + 1),
        for the same stop s: the stop is a discontinuous decision, so the fixtures keep every |P_i| examined a
        thousand bounds away from 0 (the generator asserts it and moves to another seed otherwise).
ess     (m L) / tau: relative E_tau / |tau| to first order (1.01 covers the second) and a rounding; cap carries the
        host's log10 and a product (4 u cap covers both and the division's rounding); min moves by no more than its
        arguments, and where (m L) / tau > 2 cap the cap alone decides:
          E_ess = 4 u cap + [(m L) / tau <= 2 cap] 1.01 ess E_tau / |tau|.
mcse    pooled_std / sqrt(ess): E_mcse = mcse (E_std / pooled_std + 0.505 E_ess / ess + 3 u), E_std chainrhat_oracle's.
"""
import functools

import numpy as np

import chainrhat_oracle as R

LD = np.longdouble
U = R.U
OUTPUTS = ("ess", "ess_split", "tau", "tau_split", "mcse")
WINDOWS = ("window", "window_split")
ORDERS = ("forward", "reversed", "pairwise")


def lag_sums(y, K, order="pairwise"):
    """c(k) = sum_{t=0}^{L-1-k} y[t] y[t+k] for k = 0 .. K of y [L, ...] in y's dtype, as [K + 1, ...]. 'forward' and
    'reversed': every lag summed sequentially in increasing / decreasing t; 'pairwise': numpy's sum."""
    L = y.shape[0]
    c = np.zeros((K + 1,) + y.shape[1:], y.dtype)
    if order == "pairwise":
        for k in range(K + 1):
            c[k] = np.sum(y[:L - k] * y[k:], axis=0)
        return c
    for t in (range(L) if order == "forward" else range(L - 1, -1, -1)):
        # row t is the first factor of lag k for k <= L - 1 - t
        top = min(K, L - 1 - t)
        c[:top + 1] = c[:top + 1] + y[t] * y[t:t + top + 1]
    return c


def geyer(a, W, vplus, K, L, tp):
    """From a [K + 1, cols] (a(k)), W, vplus [cols]: tau, s, capped, the least |P_i| over the pairs i >= 1 examined."""
    cols = a.shape[1:]
    npairs = (K + 1) // 2
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = tp(1) - (W - a) / vplus
    rho[0] = tp(1)
    s = np.full(cols, npairs, np.int64)
    stopped = np.zeros(cols, bool)
    Q = rho[0] + rho[1]
    tot = Q.copy()
    margin = np.full(cols, np.inf)
    for i in range(1, npairs):
        P = rho[2 * i] + rho[2 * i + 1]
        live = ~stopped
        with np.errstate(invalid="ignore"):
            stop = live & ~(P > 0)
            margin = np.where(live, np.fmin(margin, np.abs(P).astype(np.float64)), margin)
            s = np.where(stop, i, s)
            stopped |= stop
            Qn = np.where(P < Q, P, Q)
        go = ~stopped
        Q = np.where(go, Qn, Q)
        tot = np.where(go, tot + Qn, tot)
        if stopped.all():
            break
    capped = ~stopped & (K < L - 1)
    with np.errstate(invalid="ignore"):
        tau = np.where(capped, tp(np.inf), tp(-1) + tp(2) * tot)
    return tau, s, capped, margin


def table(chain, s2chain=None, npar=None, group=None, max_lag=0, dtype=np.float64, order="pairwise"):
    """The outputs of tci_chainess for chain [rows, n_chains, ld] as arrays [n_groups, ld + 1] (s2 is the last column)
    in `dtype`, the windows as int32, and what the bounds need (W, T, vplus, cap, s, margin per variant, X, M and the
    chainrhat table under 'rhat')."""
    chain = np.asarray(chain, np.float64)
    n, nc, ld = chain.shape
    npar = np.full(nc, ld) if npar is None else np.broadcast_to(np.asarray(npar), (nc,))
    group = np.zeros(nc, np.int64) if group is None else np.asarray(group)
    ng = max(int(group.max()) + 1, 1)
    rh = R.table(chain, s2chain, npar, group, dtype=dtype, order=order)
    x = np.full((n, nc, ld + 1), np.nan)
    x[:, :, :ld] = chain
    if s2chain is not None:
        x[:, :, ld] = np.asarray(s2chain, np.float64).reshape(n, nc)
    live = np.arange(ld + 1)[None, :] < npar[:, None]
    live[:, ld] = s2chain is not None
    bad = ~np.all(np.isfinite(x), axis=0) | ~live
    xs = np.where(bad[None], 0.0, x).astype(dtype)
    h = n // 2
    tp = np.dtype(dtype).type
    with np.errstate(invalid="ignore", divide="ignore"):
        mom = [R.seq_moments(xs, order), R.seq_moments(xs[:h], order), R.seq_moments(xs[n - h:], order)]
    out = {k: np.full((ng, ld + 1), np.nan, dtype) for k in OUTPUTS}
    for k in WINDOWS:
        out[k] = np.full((ng, ld + 1), -1, np.int32)
    for k in ("W", "T", "vplus", "cap", "margin"):
        for sfx in ("", "_split"):
            out[k + sfx] = np.full((ng, ld + 1), np.nan)
    out["rhat"], out["X"], out["M"] = rh, rh["X"], rh["M"]
    for g in range(ng):
        cs = np.nonzero(group == g)[0]
        M = len(cs)
        if M == 0:
            continue
        ok = ~np.any(bad[cs], axis=0)
        for split in (0, 1):
            sfx = "_split" if split else ""
            L, m = (h, 2 * M) if split else (n, M)
            if L < 2:
                out["window" + sfx][g] = np.where(ok, 0, -1)
                continue
            seqs = [(c, q) for c in cs for q in ((1, 2) if split else (0,))]
            mu = np.stack([mom[q][0][c] for c, q in seqs])
            s2 = np.stack([mom[q][1][c] for c, q in seqs])
            _, sv, _, dev, W, T = R.psrf(mu, s2, L)
            if m < 2:
                T = np.zeros_like(W)
            vplus = (tp(L - 1) / tp(L)) * W + T
            K = L - 1 if max_lag == 0 else min(int(max_lag), L - 1)
            acc = np.zeros((K + 1, ld + 1), dtype)
            for (c, q), muj in zip(seqs, mu):
                r0 = n - h if q == 2 else 0
                y = xs[r0:r0 + L, c] - muj
                acc = acc + lag_sums(y, K, order) / tp(L)
            a = acc / tp(m)
            tau, s, _, margin = geyer(a, W, vplus, K, L, tp)
            mL = tp(m * L)
            cap = mL * np.log10(mL)
            with np.errstate(invalid="ignore", divide="ignore"):
                q_ = mL / tau
                ess = np.where(np.isnan(tau), tp(np.nan), np.where(tau > 0, np.minimum(q_, cap), cap))
            out["tau" + sfx][g] = np.where(ok, tau, np.nan)
            out["ess" + sfx][g] = np.where(ok, ess, np.nan)
            out["window" + sfx][g] = np.where(ok, 2 * s, -1)
            if not split:
                with np.errstate(invalid="ignore", divide="ignore"):
                    out["mcse"][g] = np.where(ok, rh["pooled_std"][g] / np.sqrt(ess), np.nan)
            for k, v in (("W", W), ("T", T), ("vplus", vplus), ("margin", margin)):
                out[k + sfx][g] = np.where(ok, np.asarray(v, np.float64), np.nan)
            out["cap" + sfx][g] = np.where(ok, float(cap), np.nan)
    return out


def bounds(ref, n):
    """The bounds of the module docstring from the longdouble table `ref`: E_P, E_tau, E_ess per variant and E_mcse,
    [n_groups, ld + 1] each."""
    f = lambda a_: np.asarray(a_, np.float64)  # noqa: E731
    X, M = ref["X"], ref["M"][:, None].astype(np.float64)
    b = {}
    for split in (0, 1):
        sfx = "_split" if split else ""
        L, m = (n // 2, 2 * M) if split else (n, M)
        if L < 2:
            for k in ("P", "tau", "ess"):
                b[k + sfx] = np.zeros_like(X)
            continue
        lam = L / (L - 1.0)
        W, T, vp = ref["W" + sfx], ref["T" + sfx], ref["vplus" + sfx]
        tau, ess, cap = f(ref["tau" + sfx]), f(ref["ess" + sfx]), ref["cap" + sfx]
        s = ref["window" + sfx] / 2.0
        with np.errstate(invalid="ignore", divide="ignore"):
            Ea = 8 * U * X * np.sqrt(W) + (L + m + 6) * U * W + 36 * (U * X) ** 2
            EWa = Ea + (L + m + 5) * U * W + 32 * (U * X) ** 2
            Ev = (L + 2 * m + 10) * U * vp + 12 * U * X * np.sqrt(T) + (2 * m * m + 96) * (U * X) ** 2
            Erho = (EWa + 2 * lam * Ev) / vp + (4 * lam + 1) * U
            EP = 2 * Erho + (2 + 4 * lam) * U
            Etau = np.where(np.isinf(tau), 0.0, 2 * s * EP + (s + 2) * U * (np.abs(tau) + 1))   # +Inf is exact
            a = m * L / tau
            rel = np.where(np.isfinite(tau), Etau / np.abs(tau), 0.0)
            Eess = 4 * U * cap + np.where((tau > 0) & (a <= 2 * cap), 1.01 * ess * rel, 0.0)
        b["P" + sfx], b["tau" + sfx], b["ess" + sfx] = EP, Etau, Eess
    rb = R.bounds(ref["rhat"], n)
    std, mcse, ess = f(ref["rhat"]["pooled_std"]), f(ref["mcse"]), f(ref["ess"])
    with np.errstate(invalid="ignore", divide="ignore"):
        b["mcse"] = mcse * (rb["pooled_std"] / std + 0.505 * b["ess"] / ess + 3 * U)
    return b


def joined(ce):
    """A ChainEss as the table's arrays [n_groups, ld + 1]."""
    return {k: np.concatenate([getattr(ce, k), getattr(ce, "s2_" + k)[:, None]], axis=1) for k in OUTPUTS + WINDOWS}


def check(got, ref, n, where=""):
    """`got` against the longdouble table `ref`: the windows equal everywhere, NaN and Inf where and only where the
    reference has them, every finite value within its bound. Returns the largest error in units of its bound per
    output."""
    bnd = bounds(ref, n)
    for k in WINDOWS:
        assert np.array_equal(np.asarray(got[k]), ref[k]), (where, k, np.asarray(got[k]), ref[k])
    worst = {}
    for k in OUTPUTS:
        g, w = np.asarray(got[k], np.float64), np.asarray(ref[k]).astype(np.float64)
        assert g.shape == w.shape, (where, k, g.shape, w.shape)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (where, k, "NaN pattern")
        assert np.array_equal(np.isposinf(g), np.isposinf(w)) and np.array_equal(np.isneginf(g), np.isneginf(w)), \
            (where, k, "Inf pattern")
        ok = np.isfinite(w)
        err = np.abs(g[ok].astype(LD) - np.asarray(ref[k])[ok]).astype(np.float64)
        tol = bnd[k][ok]
        assert np.all(np.isfinite(tol)), (where, k, "bound not finite")
        ratio = err / np.maximum(tol, 1e-300)
        assert np.all(err <= tol), (where, k, float(np.max(ratio)))
        worst[k] = float(np.max(ratio, initial=0.0))
    return worst


def margins_hold(ref, n):
    """Every pair examined is at least 1,000 bounds away from the stop: the least |P_i| of each column that has a
    finite or infinite tau against E_P."""
    bnd = bounds(ref, n)
    for sfx in ("", "_split"):
        tau, mg, EP = np.asarray(ref["tau" + sfx], np.float64), ref["margin" + sfx], bnd["P" + sfx]
        sel = ~np.isnan(tau) & np.isfinite(mg)
        if np.any(mg[sel] <= 1000 * EP[sel]):
            return False
    return True


# ---- fixtures shared by the host and the device tests ----------------------------------------------------------

def ar1_chains(seed, rows, n_chains, ld, npar, phi=None, shift=0.3):
    """AR(1) chains [rows, n_chains, ld] and s2 [rows, n_chains]: per column a seeded phi in [0, 0.99) (or `phi`), a
    scale between 1e-2 and 1e2, a mean within a few units of 0 and a per-chain shift of `shift` standard deviations
    (so that T > 0). Padding columns (j >= npar) hold values that are not 0."""
    rng = np.random.default_rng(seed)
    ph = rng.uniform(0.0, 0.99, ld) if phi is None else np.full(ld, float(phi))
    scale = 10.0 ** rng.uniform(-2.0, 2.0, ld)
    mean = rng.standard_normal(ld)
    e = rng.standard_normal((rows, n_chains, ld + 1))
    x = np.empty((rows, n_chains, ld + 1))
    x[0] = e[0]
    phs = np.concatenate([ph, [0.5]])
    for t in range(1, rows):
        x[t] = phs * x[t - 1] + np.sqrt(1 - phs ** 2) * e[t]
    off = shift * rng.standard_normal((n_chains, ld))
    ch = mean + scale * (x[:, :, :ld] + off[None])
    for c, P in enumerate(npar):
        ch[:, c, int(P):] = 7.0 + rng.standard_normal((rows, ld - int(P)))
    s2 = 2.0 + 0.3 * x[:, :, ld]
    return np.ascontiguousarray(ch), np.ascontiguousarray(s2)


# n on both sides of what the kernels tile by: the moments' 8 / 32-row steps and 256-row segments (tci_chainrhat's,
# reused) and k_ce_lags' 32-row tiles and 64-lag tiles, for the whole chain (n) and for the halves (h = n // 2:
# n = 63 .. 66 puts h around 32, 127 .. 131 around 64, 511 .. 514 around 256); the largest is 1,100.
NS = (1, 2, 3, 4, 5, 7, 8, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 131, 255, 256, 257, 511, 513, 514, 1100)
LDS = (1, 63, 64, 65, 130)
MS = (1, 2, 3, 4, 7)
MAX_LAGS = (0, 1, 2, 3, 64, 65)


def _shape(i):
    n = NS[i]
    # the wide ld go to the short chains: the restatement's lag sums cost n^2 x chains x ld
    ld = LDS[i % len(LDS)] if n <= 66 else (1, 3, 2)[i % 3]
    sizes = [MS[(i + k) % len(MS)] for k in (0, 2, 3)] if n <= 66 else [MS[i % len(MS)], 2]
    np_g = [ld, max(1, ld - 3), max(1, (ld + 1) // 2)][:len(sizes)]
    return n, ld, sizes, np_g


def shape_case(i, seed_step=0):
    """Case i of the shape sweep: n = NS[i], ld, group sizes and max_lag cycling through LDS, MS and MAX_LAGS, ragged
    npar across the groups, two chains in no group; even i: the chains shuffled (groups interleave) and an s2 chain;
    odd i: the groups in descending id order and no s2 chain."""
    n, ld, sizes, np_g = _shape(i)
    rng = np.random.default_rng(1000 + i)
    ids = np.concatenate([np.full(m, g) for g, m in enumerate(sizes)] + [np.full(2, -1)])
    ids = rng.permutation(ids) if i % 2 == 0 else np.sort(ids)[::-1]
    npar = np.array([np_g[g] if g >= 0 else ld for g in ids], np.int32)
    chain, s2 = ar1_chains(3000 + i + 100 * seed_step, n, len(ids), ld, npar)
    return {"name": f"n{n}_ld{ld}_M{'-'.join(map(str, sizes))}_lag{MAX_LAGS[i % len(MAX_LAGS)]}", "chain": chain,
            "s2": s2 if i % 2 == 0 else None, "npar": npar, "group": np.ascontiguousarray(ids, np.int32), "n": n,
            "max_lag": MAX_LAGS[i % len(MAX_LAGS)]}


def special_case():
    """M = 3 chains of 300 rows, 10 columns: 0 AR(1); 1 the same constant in every chain (vplus = 0: NaN); 2 constant
    in chain 0 only; 3 a different constant per chain (W = 0 < T: every rho is 1, tau = 2 n - 1); 4 a NaN, 5 a +Inf
    and 8 a -Inf in one chain; 6 identical in the three chains; 7 alternating +-1 in every chain (tau < 0: ess is the
    cap); 9 AR(1)."""
    chain, s2 = ar1_chains(77, 300, 3, 10, [10, 10, 10])
    chain[:, :, 1] = 2.5
    chain[:, 0, 2] = -1.25
    chain[:, :, 3] = np.array([1.0, 2.0, 4.0])[None]
    chain[17, 1, 4] = np.nan
    chain[299, 2, 5] = np.inf
    chain[0, 0, 8] = -np.inf
    chain[:, :, 6] = chain[:, :1, 6]
    chain[:, :, 7] = (1.0 - 2.0 * (np.arange(300) % 2))[:, None]
    return {"name": "special", "chain": chain, "s2": s2, "npar": np.full(3, 10, np.int32),
            "group": np.zeros(3, np.int32), "n": 300, "max_lag": 0}


def capped_case():
    """M = 2 strongly correlated chains of 400 rows with max_lag = 9: no pair stops within the cap (+Inf / 0)."""
    chain, s2 = ar1_chains(91, 400, 2, 3, [3, 3], phi=0.98)
    return {"name": "capped", "chain": chain, "s2": s2, "npar": np.full(2, 3, np.int32),
            "group": np.zeros(2, np.int32), "n": 400, "max_lag": 9}


def with_ref(make):
    """The case `make(step)` gives for the first step = 0, 1, .. whose every examined pair is 1,000 bounds from the
    stop, with its longdouble table under 'ref': no case is left out and no tolerance softens the stop."""
    for step in range(20):
        c = make(step)
        c["ref"] = table(c["chain"], c["s2"], c["npar"], c["group"], c["max_lag"], dtype=LD)
        if margins_hold(c["ref"], c["n"]):
            return c
    raise AssertionError("no seed keeps the pairs away from the stop")


@functools.lru_cache(maxsize=None)
def all_cases():
    """Every fixture with its reference, computed once and shared (read-only)."""
    cases = [with_ref(functools.partial(shape_case, i)) for i in range(len(NS))]
    for fixed in (special_case(), capped_case()):
        c = with_ref(lambda step, fixed=fixed: dict(fixed))
        cases.append(c)
    return tuple(cases)
