"""numpy restatement of tci_modesearch (include/tci.h) for the tests: DE/rand/1/bin on f = ss / s2 + pri over one cell's
population, with the SS function passed in. float64 throughout, every operation rounded once in the stated order, so
with the likelihood kernel as the SS function every output is the device's bits. Philox is tests/temper_oracle.py's,
the prior sum tests/chainlp_oracle.py's. Host only: numpy."""
import functools

import numpy as np

import chainlp_oracle as lpo
import temper_oracle as tpo

P_INDEX, P_CROSS = 7, 8
M32 = 0xFFFFFFFF


@functools.lru_cache(maxsize=1 << 18)
def rng(seed, key, step, purpose, idx):
    """The sampler's counter layout (key, step, purpose, idx) under the key (seed): four 32-bit words."""
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step)
    return tuple(tpo.philox4x32_10([int(key) & M32, step & M32, ((step >> 32) & 0x00FFFFFF) | (purpose << 24),
                                    int(idx) & M32], [seed & M32, seed >> 32]))


def u01(a, b):
    return (float(((a << 32) | b) >> 11) + 0.5) * 2.0 ** -53


def scale(w, n):
    """m(w, n): a 32-bit word scaled to [0, n)."""
    return (w * n) >> 32


def index_draw(seed, key, g, i, n_pop, P):
    """(r1, r2, r3, jrand) of member i in generation g."""
    w = rng(seed, key, g, P_INDEX, i)
    r1 = scale(w[0], n_pop - 1)
    r1 += r1 >= i
    r2 = scale(w[1], n_pop - 2)
    for e in sorted((i, r1)):
        r2 += r2 >= e
    r3 = scale(w[2], n_pop - 3)
    for e in sorted((i, r1, r2)):
        r3 += r3 >= e
    return int(r1), int(r2), int(r3), int(scale(w[3], P))


def cross_uniforms(seed, key, g, i, P):
    """u_j, j < P: words (x, y) of call i * 2048 + (j >> 1) for even j, (z, w) for odd j."""
    u = np.empty(P)
    for j in range(P):
        c = rng(seed, key, g, P_CROSS, i * 2048 + (j >> 1))
        u[j] = u01(c[2], c[3]) if j & 1 else u01(c[0], c[1])
    return u


def trial(x, i, r1, r2, r3, jrand, u, P, lower, upper, F, CR):
    """The trial row of member i of the population x [n_pop, ld]; entries j >= P are the parent's."""
    with np.errstate(all="ignore"):
        d = x[r2, :P] - x[r3, :P]
        s = np.float64(F) * d
        v = x[r1, :P] + s
        cross = (u < CR) | (np.arange(P) == jrand)
        take = cross & (v >= lower[:P]) & (v <= upper[:P])   # a NaN mutant fails both comparisons
    t = x[i].copy()
    t[:P] = np.where(take, v, x[i, :P])
    return t


def objective(ss, pri, s2):
    with np.errstate(all="ignore"):
        return np.asarray(ss, np.float64) / np.float64(s2) + pri


def best_index(f):
    """First in the order (f is NaN, f, index)."""
    f = np.asarray(f, np.float64)
    if np.all(np.isnan(f)):
        return 0
    return int(np.nanargmin(f))   # the first of the least


def search(ss_fn, pop0, P, lower, upper, mu, sig, s2=1.0, key=0, seed=0, n_gen=3, F=0.5, CR=0.9):
    """One cell's search. ss_fn(rows [n, ld]) -> ss [n]; pop0 [n_pop, ld]; lower, upper, mu, sig [>= P]. Returns a dict
    of pop, f, ss, pri, best, theta_best (padding NaN), f_best, ss_best, pri_best, f_trace [n_gen + 1], n_accepted
    [n_gen]."""
    x = np.array(pop0, np.float64)
    n_pop, ld = x.shape
    ss = np.asarray(ss_fn(x), np.float64).copy()
    pri = np.asarray(lpo.pri(x[:, :P], mu[:P], sig[:P]), np.float64).copy()
    f = objective(ss, pri, s2)
    trace, nacc = [f[best_index(f)]], []
    for g in range(1, int(n_gen) + 1):
        t = np.empty_like(x)
        for i in range(n_pop):
            r1, r2, r3, jrand = index_draw(seed, key, g, i, n_pop, P)
            t[i] = trial(x, i, r1, r2, r3, jrand, cross_uniforms(seed, key, g, i, P), P, lower, upper, F, CR)
        ss_t = np.asarray(ss_fn(t), np.float64)
        pri_t = lpo.pri(t[:, :P], mu[:P], sig[:P])
        f_t = objective(ss_t, pri_t, s2)
        with np.errstate(invalid="ignore"):
            take = f_t <= f   # a NaN f_trial never replaces
        x[take], f[take], ss[take], pri[take] = t[take], f_t[take], ss_t[take], pri_t[take]
        trace.append(f[best_index(f)])
        nacc.append(int(take.sum()))
    b = best_index(f)
    tb = np.full(ld, np.nan)
    tb[:P] = x[b, :P]
    return dict(pop=x, f=f, ss=ss, pri=pri, best=b, theta_best=tb, f_best=f[b], ss_best=ss[b], pri_best=pri[b],
                f_trace=np.array(trace), n_accepted=np.array(nacc, np.int32))
