"""numpy restatement of tci_demc_run (include/tci.h) for the tests: the DE-MC population sampler of one cell, with the SS
function passed in. float64 throughout, every operation rounded once in the stated order, so with the likelihood kernel
as the SS function every output but the ones behind exp and the Gamma variate's log, cos and sqrt is the device's bits.
The one inexact decision is u < exp(logr): the restatement calls it decidable when |u - exp(logr)| > EXP_MARGIN *
exp(logr) and reports the others; EXP_MARGIN = 16 * 2^-53 covers fitcheck_oracle.K_EXP = 3 ulp = 6 * 2^-53 of the device
library plus the host libm's ulp. Philox is tests/temper_oracle.py's (vectorised here for the coordinate draws), the
prior sum tests/chainlp_oracle.py's. Host only: numpy."""
import math

import numpy as np

import chainlp_oracle as lpo
import modesearch_oracle as mso

P_INDEX, P_COORD, P_ACCEPT, P_SIGMA = 9, 10, 11, 12
M32 = 0xFFFFFFFF
EXP_MARGIN = 16.0 * 2.0 ** -53

rng, u01, scale = mso.rng, mso.u01, mso.scale


def rng_vec(seed, key, step, purpose, idx):
    """rng(seed, key, step, purpose, idx) for an array of idx: four uint64 arrays holding 32-bit words."""
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step)
    idx = np.asarray(idx, np.uint64)
    m = np.uint64(M32)
    c = [np.full(idx.shape, int(key) & M32, np.uint64), np.full(idx.shape, step & M32, np.uint64),
         np.full(idx.shape, ((step >> 32) & 0x00FFFFFF) | (purpose << 24), np.uint64), idx & m]
    k0, k1 = seed & M32, seed >> 32
    s = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> s) ^ c[1] ^ np.uint64(k0), p1 & m, (p0 >> s) ^ c[3] ^ np.uint64(k1), p0 & m]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c


def u01_vec(a, b):
    return ((((a << np.uint64(32)) | b) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def index_draw(seed, key, step, i, h, n_pop, P):
    """(r1, r2, jrand) of moving member i in half-sweep h: the pair from the resting members 1 - h, 3 - h, .."""
    n_mov = (n_pop - h + 1) // 2
    n_rest = n_pop - n_mov
    w = rng(seed, key, step, P_INDEX, i)
    a = scale(w[0], n_rest)
    c = scale(w[1], n_rest - 1)
    c += c >= a
    return int(2 * a + 1 - h), int(2 * c + 1 - h), int(scale(w[2], P))


def coord_uniforms(seed, key, step, i, P):
    """(u_j, v_j), j < P: words (x, y) and (z, w) of call i * 4096 + j."""
    q = rng_vec(seed, key, step, P_COORD, i * 4096 + np.arange(P))
    return u01_vec(q[0], q[1]), u01_vec(q[2], q[3])


def trial(x, i, r1, r2, jrand, u, v, P, lower, upper, jitter, CR, gamma0, jump):
    """(trial row, oob, d') of member i of the population x [n_pop, ld]; entries j >= P are the parent's."""
    cross = np.ones(P, bool) if jump else (u < CR) | (np.arange(P) == jrand)
    dp = int(cross.sum())
    gam = np.float64(1.0) if jump else np.float64(gamma0) / np.sqrt(np.float64(2 * dp))
    with np.errstate(all="ignore"):
        d = x[r1, :P] - x[r2, :P]
        s = gam * d
        y = x[i, :P] + s
        e = 2.0 * v
        f = e - 1.0
        z = jitter[:P] * f
        tj = y + z
        bad = cross & ~((tj >= lower[:P]) & (tj <= upper[:P]))   # a NaN fails both comparisons
    t = x[i].copy()
    t[:P] = np.where(cross, tj, x[i, :P])
    return t, bool(bad.any()), dp


def gamma_unit(seed, key, step, a, purpose, base):
    """The sampler's Marsaglia-Tsang unit variate (tci_gamma.h; oracle/tci_dram_oracle.c's gamma_unit) on the calls
    base | it and base | it | 2^31 of stream (seed, key, step, purpose)."""
    d = a - 1.0 / 3.0
    cc = 1.0 / math.sqrt(9.0 * d)
    for it in range(1024):
        r = rng(seed, key, step, purpose, base | it)
        u1, u2 = u01(r[0], r[1]), u01(r[2], r[3])
        x = math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * math.pi * u2)
        r2 = rng(seed, key, step, purpose, base | it | 0x80000000)
        u = u01(r2[0], r2[1])
        v = 1.0 + cc * x
        if v <= 0.0:
            continue
        v = v * v * v
        x2 = x * x
        if u < 1.0 - 0.0331 * x2 * x2:
            return d * v
        if math.log(u) < 0.5 * x2 + d - d * v + d * math.log(v):
            return d * v
    return a


def run(ss_fn, pop0, P, lower, upper, mu, sig, jitter, sigma2_0=1.0, key=0, seed=0, n_gen=3, thin=1, jump_every=0,
        CR=0.2, gamma0=0.0, updatesigma=False, forced_s2=None):
    """One cell's run. ss_fn(rows [n, ld]) -> ss [n]; pop0 [n_pop, ld]; lower, upper, mu, sig, jitter [>= P].
    forced_s2 [n_gen + 1, n_pop] (needs updatesigma): after member i's own draw in generation g, recorded in s2_draw
    [n_gen, n_pop], its s2 is set to forced_s2[g, i] (the device's), so that the decisions replay.
    Returns a dict of chain, s2chain, sschain, prichain (kept rows), pop, s2, ss, pri, accept_rate, n_oob, n_evals, logr,
    accepted, trial_oob [n_gen, n_pop], s2_draw and undecided: the (g, i) whose u < exp(logr) is within EXP_MARGIN."""
    x = np.array(pop0, np.float64)
    n_pop, ld = x.shape
    N = P - 7
    gamma0 = 2.38 if gamma0 <= 0 else gamma0
    ss = np.asarray(ss_fn(x), np.float64).copy()
    pri = np.asarray(lpo.pri(x[:, :P], mu[:P], sig[:P]), np.float64).copy()
    s2 = np.full(n_pop, np.float64(sigma2_0))
    nacc, noob = np.zeros(n_pop, np.int64), np.zeros(n_pop, np.int64)
    logr = np.full((n_gen, n_pop), np.nan)
    acc, oobl = np.zeros((n_gen, n_pop), np.uint8), np.zeros((n_gen, n_pop), np.uint8)
    s2_draw = np.full((n_gen, n_pop), np.nan)
    undecided = []
    kept = {k: [] for k in ("chain", "s2chain", "sschain", "prichain")}

    def keep():
        for k, a in zip(("chain", "s2chain", "sschain", "prichain"), (x, s2, ss, pri)):
            kept[k].append(a.copy())

    if thin > 0:
        keep()
    for g in range(1, int(n_gen) + 1):
        jump = jump_every > 0 and g % jump_every == 0
        for h in (0, 1):
            step = 2 * g + h
            movers = list(range(h, n_pop, 2))
            t = np.empty((len(movers), ld))
            oob = np.zeros(len(movers), bool)
            for q, i in enumerate(movers):
                r1, r2, jrand = index_draw(seed, key, step, i, h, n_pop, P)
                u, v = coord_uniforms(seed, key, step, i, P)
                t[q], oob[q], _ = trial(x, i, r1, r2, jrand, u, v, P, lower, upper, jitter, CR, gamma0, jump)
            ss_t = np.full(len(movers), np.inf)
            if (~oob).any():   # a proposal rejected at the bounds is never evaluated
                ss_t[~oob] = np.asarray(ss_fn(t[~oob]), np.float64)
            pri_t = lpo.pri(t[:, :P], mu[:P], sig[:P])
            for q, i in enumerate(movers):
                take = False
                if oob[q]:
                    noob[i] += 1
                    oobl[g - 1, i] = 1
                else:
                    with np.errstate(all="ignore"):
                        fo = ss[i] / s2[i] + pri[i]
                        fn = ss_t[q] / s2[i] + pri_t[q]
                        lr = np.float64(-0.5) * (fn - fo)
                    logr[g - 1, i] = lr
                    if lr >= 0:
                        take = True
                    elif lr == lr:
                        w = rng(seed, key, step, P_ACCEPT, i)
                        uu, e = u01(w[0], w[1]), math.exp(lr)
                        take = uu < e
                        if not abs(uu - e) > EXP_MARGIN * e:
                            undecided.append((g, i))
                if take:
                    x[i], ss[i], pri[i] = t[q], ss_t[q], pri_t[q]
                    nacc[i] += 1
                    acc[g - 1, i] = 1
                if updatesigma:
                    with np.errstate(all="ignore"):
                        gu = gamma_unit(seed, key, step, float(N), P_SIGMA, i << 16)
                        s2[i] = 1.0 / (gu * (2.0 / ss[i]))
                    s2_draw[g - 1, i] = s2[i]
                    if forced_s2 is not None:
                        s2[i] = forced_s2[g, i]
        if thin > 0 and g % thin == 0:
            keep()
    out = {k: np.array(v) for k, v in kept.items()}
    out.update(pop=x, s2=s2, ss=ss, pri=pri, accept_rate=nacc / n_gen if n_gen else np.full(n_pop, np.nan), n_oob=noob,
               n_evals=1 + n_gen - noob, logr=logr, accepted=acc, trial_oob=oobl, s2_draw=s2_draw, undecided=undecided)
    return out


def ess_multi(x):
    """The multi-chain effective sample size (BDA3 11.5) of x [rows, members] in plain numpy: the members' mean
    autocorrelation against the pooled variance, summed by Geyer's initial positive sequence."""
    n, m = x.shape
    y = x - x.mean(axis=0)
    W = y.var(axis=0, ddof=1).mean()
    vp = (n - 1) / n * W + x.mean(axis=0).var(ddof=1)
    rho = [1.0] + [1 - (W - (y[:n - k] * y[k:]).sum(axis=0).mean() / n) / vp for k in range(1, n - 1)]
    tau = -1.0
    for i in range(0, len(rho) - 1, 2):
        p = rho[i] + rho[i + 1]
        if not p > 0:
            break
        tau += 2 * p
    return n * m / max(tau, 1.0 / (n * m))


def gaussian_target(P, n_pop, seed):
    """The target of the distribution tests on a cell of P parameters: N(mu, sig^2) per coordinate inside bounds at
    mu +- 8 sig, mu the centre and sig 1/16 of the width of cell_setup's box; pop0 drawn from the target itself."""
    lo = np.concatenate([[0, 0, 0, 0, 0, 0, 0], np.full(P - 7, -30.0)])
    up = np.concatenate([[10, 20, 10, 50, 50, 1, 40], np.full(P - 7, 30.0)])
    mu, sig = (lo + up) / 2, (up - lo) / 16
    pop0 = mu + sig * np.random.default_rng(seed).standard_normal((n_pop, P))
    return pop0, mu - 8 * sig, mu + 8 * sig, mu, sig


def worst_z(chain, mu, sig):
    """The largest |z| over the coordinates of the pooled mean against mu and the pooled std against sig of chain
    [rows, members, P], each in Monte-Carlo standard errors from the coordinate's own ess_multi: sig / sqrt(ess) for the
    mean and sig / sqrt(2 ess) for the std (a Gaussian's). Returns (worst z, least ess)."""
    zs, es = [], []
    for j in range(chain.shape[2]):
        x = chain[:, :, j]
        e = ess_multi(x)
        es.append(e)
        zs.append(abs(x.mean() - mu[j]) / (sig[j] / np.sqrt(e)))
        zs.append(abs(x.std() - sig[j]) / (sig[j] / np.sqrt(2 * e)))
    return max(zs), min(es)


# The distribution tests (tests/test_demc_host.py on the restatement with the C oracle's SS, tests/test_demc_gpu.py on
# the device, the same constants). Sized on the restatement: with 64 members a 120-dimensional Gaussian mixes slowly (the
# members' differences span 63 directions), 600 generations give an ESS of 50 to 100 per coordinate, and the restatement's
# worst |z| over the 240 statistics is recorded beside the host test; TARGET_Z leaves it a margin of 2.
TARGET = dict(n_pop=64, n_gen=600, n_burn=100, CR=0.1, jitter=0.01, sigma2_0=1e12, seed=3, pop_seed=5)
TARGET_Z = 5.0
