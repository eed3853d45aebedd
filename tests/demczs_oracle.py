"""numpy restatement of tci_demczs_run (include/tci.h) for the tests: the DE-MC(zs) sampler of one cell, with the SS
function passed in; built on tests/demc_oracle.py (Philox, the parallel trial, the Gamma variate, EXP_MARGIN) and
tests/chainlp_oracle.py (the prior sum). float64 throughout, every operation rounded once in the stated order.

The inexact steps are exp, as in demc_oracle, and the two log calls of a snooker move's ljac. The restatement computes
its own ljac and reports it (ljac_own) with a bound (ljac_bound), then carries on with the device's bits when they are
given (forced_ljac, as forced_s2 does for sigma2), so that every other output replays bit for bit. The bound, with
u = 2^-53, h = (P - 1) / 2 (exact in float64) and L = |log D'| + |log D|:
  each log   the device library's error is at most chainlp_oracle.K_LOG = 3 ulp and the host libm's at most 1 ulp, and an
             ulp is at most 2 u relative: the two values of one log differ by at most 2 (K_LOG + 1) u |log|;
  the difference  either side rounds its own subtraction once, u |dl| each and |dl| <= L: together (2 K_LOG + 4) u L;
  times h    either side rounds the product once, u |ljac| each with |ljac| <= h L (1 + 8 u): 2 u h L more.
|ljac_device - ljac_own| <= LJAC_U * u * h * L with LJAC_U = 1.01 * (2 K_LOG + 6) = 12.12. D and D' themselves are
exact restatements (the butterfly sum below), so both sides take the logs of the same bits. A ljac that is not finite
(D' = 0 gives -Inf) must be the device's bit for bit.
A decision within demc_oracle.EXP_MARGIN of u = exp(logr) is reported in `undecided`. Host only: numpy."""
import math

import numpy as np

import chainlp_oracle as lpo
import demc_oracle as dmo

P_INDEX, P_COORD, P_ACCEPT, P_SIGMA = 13, 14, 15, 16
U = 2.0 ** -53
LJAC_U = 1.01 * (2 * lpo.K_LOG + 6)
EXP_MARGIN = dmo.EXP_MARGIN
LANES = 64
MAX_POP = 4096

rng, u01, scale = dmo.rng, dmo.u01, dmo.scale


def sum64(terms):
    """The defined order of D, A and D' for terms [P] or [B, P]: lane l adds its terms j = l, l + 64, .. ascending from
    0.0, then the 64 partials combine by the xor butterfly p <- p + p[lane ^ d], d = 32 .. 1: six pairwise folds, every
    lane the same value."""
    t = np.asarray(terms, np.float64)
    one = t.ndim == 1
    t = np.atleast_2d(t)
    B, n = t.shape
    R = -(-n // LANES)
    pad = np.zeros((B, R * LANES))      # a missing term adds +0.0 to a partial that started at +0.0: no bit changes
    pad[:, :n] = t
    with np.errstate(all="ignore"):
        p = np.zeros((B, LANES))
        for r in range(R):
            p = p + pad[:, r * LANES:(r + 1) * LANES]
        lane = np.arange(LANES)
        for d in (32, 16, 8, 4, 2, 1):
            p = p + p[:, lane ^ d]
    return np.float64(p[0, 0]) if one else p[:, 0].copy()


def sum64_loops(terms):
    """sum64 spelled out lane by lane in plain Python (the host test holds the two together)."""
    part = [0.0] * LANES
    for j, x in enumerate(terms):
        part[j % LANES] = part[j % LANES] + float(x)
    for d in (32, 16, 8, 4, 2, 1):
        part = [part[l] + part[l ^ d] for l in range(LANES)]
    return part[0]


def scale_rule(wx, wy, ww, M):
    """(a, c, e) from the three words by the scaling rule alone."""
    a = scale(wx, M)
    c = scale(wy, M - 1)
    c += c >= a
    e = scale(ww, M - 2)
    e += e >= min(a, c)
    e += e >= max(a, c)
    return int(a), int(c), int(e)


def archive_rows(g, m0, n_pop, append_every):
    """M_g: the archive rows generation g reads."""
    return m0 + n_pop * ((g - 1) // append_every)


def index_draw(seed, key, g, i, M, P, p_snooker):
    """(a, c, e, jrand, snooker, gamma_s) of chain i in generation g with M archive rows."""
    w = rng(seed, key, g, P_INDEX, i)
    q = rng(seed, key, g, P_INDEX, MAX_POP + i)
    a, c, e = scale_rule(w[0], w[1], w[3], M)
    return a, c, e, int(scale(w[2], P)), bool(u01(q[0], q[1]) < p_snooker), np.float64(1.2) + np.float64(u01(q[2], q[3]))


def index_draws(seed, key, g, n_pop, M, P, p_snooker):
    """index_draw for every chain at once: arrays (a, c, e, jrand [int64], snooker [bool], gamma_s)."""
    i = np.arange(n_pop)
    w = dmo.rng_vec(seed, key, g, P_INDEX, i)
    q = dmo.rng_vec(seed, key, g, P_INDEX, MAX_POP + i)
    sc = lambda x, n: (x * np.uint64(n)) >> np.uint64(32)  # noqa: E731  (a word below 2^32 times n below 2^24)
    a = sc(w[0], M)
    c = sc(w[1], M - 1)
    c = c + (c >= a).astype(np.uint64)
    e = sc(w[3], M - 2)
    e = e + (e >= np.minimum(a, c)).astype(np.uint64)
    e = e + (e >= np.maximum(a, c)).astype(np.uint64)
    I = lambda x: x.astype(np.int64)  # noqa: E731, E741
    return I(a), I(c), I(e), I(sc(w[2], P)), dmo.u01_vec(q[0], q[1]) < p_snooker, 1.2 + dmo.u01_vec(q[2], q[3])


def coord_uniforms(seed, key, g, i, P):
    """(u_j, v_j), j < P, of chain i: words (x, y) and (z, w) of call i * 4096 + j on purpose 14."""
    q = dmo.rng_vec(seed, key, g, P_COORD, i * 4096 + np.arange(P))
    return dmo.u01_vec(q[0], q[1]), dmo.u01_vec(q[2], q[3])


def parallel(x, x1, x2, ii, jrand, seed, key, g, P, lower, upper, jitter, CR, gamma0, jump):
    """demc_oracle.trial for the chains ii at once: x, x1, x2 [n, ld] the chains' rows and their archive pair, jrand [n].
    Returns (trial rows [n, ld], oob [n])."""
    q = dmo.rng_vec(seed, key, g, P_COORD, np.asarray(ii)[:, None] * 4096 + np.arange(P)[None, :])
    u, v = dmo.u01_vec(q[0], q[1]), dmo.u01_vec(q[2], q[3])
    cross = np.ones(u.shape, bool) if jump else (u < CR) | (np.arange(P)[None, :] == jrand[:, None])
    dp = cross.sum(axis=1)
    gam = np.ones(len(dp)) if jump else np.float64(gamma0) / np.sqrt((2 * dp).astype(np.float64))
    with np.errstate(all="ignore"):
        d = x1[:, :P] - x2[:, :P]
        s = gam[:, None] * d
        y = x[:, :P] + s
        e = 2.0 * v
        f = e - 1.0
        z = jitter[None, :P] * f
        tj = y + z
        bad = cross & ~((tj >= lower[None, :P]) & (tj <= upper[None, :P]))   # a NaN fails both comparisons
    t = x.copy()
    t[:, :P] = np.where(cross, tj, x[:, :P])
    return t, bad.any(axis=1)


def snooker(x, z, z1, z2, gs, P, lower, upper, jac_dim=None):
    """Snooker moves of the rows x [n, ld] (or one row [ld]) along the lines through z, with the pair z1, z2 and gamma_s
    gs: (trial rows, flag, ljac, D, D'); flag 0 in bounds, 1 out of bounds, 2 a null move; ljac NaN unless flag is 0.
    jac_dim: the Jacobian's exponent is jac_dim / 2, P - 1 by the definition (the host test passes P to see the bias)."""
    one = np.ndim(x) == 1
    x, z, z1, z2 = (np.atleast_2d(np.asarray(v, np.float64)) for v in (x, z, z1, z2))
    gs = np.atleast_1d(np.asarray(gs, np.float64))
    jac_dim = P - 1 if jac_dim is None else jac_dim
    with np.errstate(all="ignore"):
        d = x[:, :P] - z[:, :P]
        D = sum64(d * d)
        A = sum64((z1[:, :P] - z2[:, :P]) * d)
        null = (D == 0) | ~np.isfinite(D)
        r = A / D
        s = gs * r
        t = x.copy()
        t[:, :P] = x[:, :P] + s[:, None] * d
        bad = (~((t[:, :P] >= lower[None, :P]) & (t[:, :P] <= upper[None, :P]))).any(axis=1)
        f = t[:, :P] - z[:, :P]
        Dp = sum64(f * f)
        h = np.float64(0.5) * np.float64(jac_dim)
        lj = h * (np.log(Dp) - np.log(D))
    flag = np.where(null, 2, np.where(bad, 1, 0))
    t[null] = x[null]
    lj = np.where(flag == 0, lj, np.nan)
    out = (t, flag, lj, D, Dp)
    return tuple(v[0] for v in out) if one else out


def ljac_bound(P, D, Dp):
    with np.errstate(all="ignore"):
        return LJAC_U * U * (0.5 * (P - 1)) * (np.abs(np.log(Dp)) + np.abs(np.log(D)))


def run(ss_fn, pop0, z0, P, lower, upper, mu, sig, jitter, sigma2_0=1.0, key=0, seed=0, n_gen=3, thin=1, jump_every=0,
        CR=0.2, gamma0=0.0, updatesigma=False, forced_s2=None, append_every=10, p_snooker=0.1, forced_ljac=None,
        jac_dim=None):
    """One cell's run. ss_fn(rows [n, ld]) -> ss [n]; pop0 [n_pop, ld]; z0 [m0, ld]; lower, upper, mu, sig, jitter [>= P].
    forced_s2 [n_gen + 1, n_pop] as demc_oracle.run's. forced_ljac [n_gen, n_pop]: the device's ljac log; an evaluated
    snooker move carries on with forced_ljac[g - 1, i] after its own value went to ljac_own and its bound to ljac_bound
    (NaN elsewhere). Returns demc_oracle.run's dict (trial_oob 2 for a null move) plus n_null, ljac (the values used),
    ljac_own, ljac_bound, snooker [n_gen, n_pop], archive [M_final, ld] and undecided."""
    x = np.array(pop0, np.float64)
    n_pop, ld = x.shape
    m0 = len(z0)
    M_final = m0 + n_pop * (int(n_gen) // append_every)
    Z = np.empty((M_final, ld))
    Z[:m0] = z0
    N = P - 7
    gamma0 = 2.38 if gamma0 <= 0 else gamma0
    ss = np.asarray(ss_fn(x), np.float64).copy()
    pri = np.asarray(lpo.pri(x[:, :P], mu[:P], sig[:P]), np.float64).copy()
    s2 = np.full(n_pop, np.float64(sigma2_0))
    nacc, noob, nnull = (np.zeros(n_pop, np.int64) for _ in range(3))
    nan = lambda: np.full((n_gen, n_pop), np.nan)  # noqa: E731
    logr, ljl, lj_own, lj_bound, s2_draw = nan(), nan(), nan(), nan(), nan()
    acc, oobl, snkl = (np.zeros((n_gen, n_pop), np.uint8) for _ in range(3))
    undecided = []
    kept = {k: [] for k in ("chain", "s2chain", "sschain", "prichain")}

    def keep():
        for k, a in zip(("chain", "s2chain", "sschain", "prichain"), (x, s2, ss, pri)):
            kept[k].append(a.copy())

    if thin > 0:
        keep()
    every = np.arange(n_pop)
    for g in range(1, int(n_gen) + 1):
        jump = jump_every > 0 and g % jump_every == 0
        M = archive_rows(g, m0, n_pop, append_every)
        a, c, e, jrand, snk, gs = index_draws(seed, key, g, n_pop, M, P, p_snooker)
        snkl[g - 1] = snk
        t = x.copy()
        flag = np.zeros(n_pop, np.int64)
        lj = np.zeros(n_pop)
        ii, si = np.flatnonzero(~snk), np.flatnonzero(snk)
        if len(ii):
            t[ii], ob = parallel(x[ii], Z[a[ii]], Z[c[ii]], ii, jrand[ii], seed, key, g, P, lower, upper, jitter, CR, gamma0,
                                 jump)
            flag[ii] = ob
        if len(si):
            t[si], flag[si], own, D, Dp = snooker(x[si], Z[e[si]], Z[a[si]], Z[c[si]], gs[si], P, lower, upper, jac_dim)
            lj[si] = own
            lj_own[g - 1, si] = own
            lj_bound[g - 1, si] = np.where(np.isfinite(own), ljac_bound(P, D, Dp), np.nan)
            if forced_ljac is not None:
                lj[si] = np.where(flag[si] == 0, forced_ljac[g - 1, si], np.nan)
        ljl[g - 1] = lj
        oobl[g - 1] = flag
        live = flag == 0
        ss_t = np.full(n_pop, np.inf)
        if live.any():   # a proposal rejected at the bounds, or a null move, is never evaluated
            ss_t[live] = np.asarray(ss_fn(t[live]), np.float64)
        pri_t = lpo.pri(t[:, :P], mu[:P], sig[:P])
        noob += flag == 1
        nnull += flag == 2
        w = dmo.rng_vec(seed, key, g, P_ACCEPT, every)
        uu = dmo.u01_vec(w[0], w[1])
        with np.errstate(all="ignore"):
            fo = ss / s2 + pri
            fn = ss_t / s2 + pri_t
            lr = np.where(live, np.float64(-0.5) * (fn - fo) + lj, np.nan)
            ex = np.exp(lr)
            take = live & ((lr >= 0) | (uu < ex))      # a NaN logr fails both comparisons
            close = live & (lr < 0) & ~(np.abs(uu - ex) > EXP_MARGIN * ex)
        logr[g - 1] = lr
        undecided += [(g, int(i)) for i in np.flatnonzero(close)]
        x[take], ss[take], pri[take] = t[take], ss_t[take], pri_t[take]
        nacc += take
        acc[g - 1] = take
        if updatesigma:
            for i in range(n_pop):
                with np.errstate(all="ignore"):
                    gu = dmo.gamma_unit(seed, key, g, float(N), P_SIGMA, i << 16)
                    s2[i] = 1.0 / (gu * (2.0 / ss[i]))
                s2_draw[g - 1, i] = s2[i]
                if forced_s2 is not None:
                    s2[i] = forced_s2[g, i]
        if g % append_every == 0:
            Z[M:M + n_pop] = x
        if thin > 0 and g % thin == 0:
            keep()
    out = {k: np.array(v) for k, v in kept.items()}
    out.update(pop=x, s2=s2, ss=ss, pri=pri, accept_rate=nacc / n_gen if n_gen else np.full(n_pop, np.nan), n_oob=noob,
               n_null=nnull, n_evals=1 + n_gen - noob - nnull, logr=logr, accepted=acc, trial_oob=oobl, snooker=snkl,
               ljac=ljl, ljac_own=lj_own, ljac_bound=lj_bound, s2_draw=s2_draw, archive=Z, undecided=undecided)
    return out


def gaussian_target(P, n_pop, m0, seed):
    """demc_oracle.gaussian_target with a starting archive: (pop0 [n_pop, P], z0 [m0, P], lower, upper, mu, sig), the
    archive drawn from the target itself and the chains starting at its first rows (m0 >= n_pop)."""
    z0, lo, up, mu, sig = dmo.gaussian_target(P, m0, seed)
    return z0[:n_pop].copy(), z0, lo, up, mu, sig


# The distribution tests (tests/test_demczs_host.py on the restatement with a constant SS, tests/test_demczs_gpu.py on
# the device with the likelihood kernel's, which sigma2_0 = 1e12 flattens to about 1e-8 in logr; the same constants).
# TARGET: P = 120, 4 chains, m0 = 10 P, every 10th of 20,000 generations kept and the first quarter dropped: 80,000
# evaluations, about DE-MC's 76,800 at demc_oracle.TARGET. The restatement's worst |z| over the 240 statistics is
# recorded beside the host test; the seed is chosen so that it stays 2 below demc_oracle.TARGET_Z.
# SMALL: P = 12 with every other move a snooker move, on which a Jacobian exponent of P in place of P - 1 must show. The
# wrong exponent tilts the target by |x - z|, about 3.5 % in every standard deviation, so the case is sized for an ESS
# above 10^4 per coordinate: 128 chains (the restatement works on all chains of a generation at once).
TARGET = dict(n_pop=4, m0=1200, n_gen=20000, thin=10, n_burn=5000, CR=0.1, jitter=0.01, sigma2_0=1e12, seed=3, pop_seed=5,
              p_snooker=0.1, append_every=10)
SMALL = dict(P=12, n_pop=128, m0=128, n_gen=8000, thin=8, n_burn=800, CR=1.0, jitter=0.01, sigma2_0=1e12, seed=3,
             pop_seed=5, p_snooker=0.5, append_every=10)
TARGET_Z = dmo.TARGET_Z
