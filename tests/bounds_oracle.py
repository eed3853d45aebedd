"""numpy restatement of tci_demczs_run_bounds (include/tci.h) for the tests: the per-coordinate bounds census and the
oriented reflection around tests/demczs_oracle.py and tests/demc_oracle.py, which are imported unchanged (the index
draws, the snooker move, the butterfly sum, Philox, the Gamma variate, the prior sum). Only the census and the reflect
rule are restated here; the generation loop is demczs_oracle.run's with the two woven in, and with mode 'reject' and no
census it must reproduce that function bit for bit (tests/test_bounds_host.py holds the two together). It takes ss and
ljac from the device as demczs_oracle does.

`oriented=False` applies PLAIN reflection: the orientation bit is neither used nor kept. That rule is not valid for this
proposal and exists for the validity test alone, which must refuse it. Host only: numpy."""
import numpy as np

import chainlp_oracle as lpo
import demc_oracle as dmo
import demczs_oracle as zso

REJECT, REFLECT = "reject", "reflect"


def step(x, orient, s, zz, lower, upper, reflect=True, oriented=True):
    """One crossing coordinate (arrays of any one shape): the raw trial t = (x + s') + zz' with s' = -s and zz' = -zz
    where the orientation bit is set, then at most one reflection. Returns (t_raw, t, orient_t, below, above, reflected):
    below / above are of the raw trial (a NaN is neither), `reflected` marks the coordinates a reflection was applied to.
    A coordinate that is still outside after its reflection (an overshoot beyond the width) stays outside: the caller's
    bounds rule rejects the proposal."""
    x, s, zz = (np.asarray(v, np.float64) for v in (x, s, zz))
    o = np.asarray(orient, bool) & bool(oriented)
    with np.errstate(all="ignore"):
        sp = np.where(o, -s, s)
        zp = np.where(o, -zz, zz)
        y = x + sp
        raw = y + zp
        below, above = raw < lower, raw > upper
        t = raw
        refl = np.zeros(np.shape(raw), bool)
        if reflect:
            e_lo = lower - raw
            t_lo = lower + e_lo
            e_up = raw - upper
            t_up = upper - e_up
            t = np.where(below, t_lo, np.where(above, t_up, raw))
            refl = below | above
    ot = (o ^ refl) if oriented else np.zeros(np.shape(raw), bool)
    return raw, t, ot.astype(np.uint8), below, above, refl


def parallel(x, orient, x1, x2, ii, jrand, seed, key, g, P, lower, upper, jitter, CR, gamma0, jump, reflect, oriented=True):
    """demczs_oracle.parallel with the orientation, the census and the reflection: x, orient, x1, x2 [n, ld]. Returns
    (trial rows [n, ld], oob [n], orient_t [n, ld], cross, below, above, reflected, outside [n, P]); `outside` marks the
    crossing coordinates that end outside the box (or NaN)."""
    q = dmo.rng_vec(seed, key, g, zso.P_COORD, np.asarray(ii)[:, None] * 4096 + np.arange(P)[None, :])
    u, v = dmo.u01_vec(q[0], q[1]), dmo.u01_vec(q[2], q[3])
    cross = np.ones(u.shape, bool) if jump else (u < CR) | (np.arange(P)[None, :] == jrand[:, None])
    dp = cross.sum(axis=1)
    gam = np.ones(len(dp)) if jump else np.float64(gamma0) / np.sqrt((2 * dp).astype(np.float64))
    with np.errstate(all="ignore"):
        d = x1[:, :P] - x2[:, :P]
        s = gam[:, None] * d
        e = 2.0 * v
        f = e - 1.0
        zz = jitter[None, :P] * f
        _, tj, ot, below, above, refl = step(x[:, :P], orient[:, :P], s, zz, lower[None, :P], upper[None, :P], reflect, oriented)
        bad = cross & ~((tj >= lower[None, :P]) & (tj <= upper[None, :P]))   # a NaN fails both comparisons
    t, o = x.copy(), orient.copy()
    t[:, :P] = np.where(cross, tj, x[:, :P])
    o[:, :P] = np.where(cross, ot, orient[:, :P])
    return t, bad.any(axis=1), o, cross, cross & below, cross & above, cross & refl, bad


def run(ss_fn, pop0, z0, P, lower, upper, mu, sig, jitter, sigma2_0=1.0, key=0, seed=0, n_gen=3, thin=1, jump_every=0,
        CR=0.2, gamma0=0.0, updatesigma=False, forced_s2=None, append_every=10, p_snooker=0.1, forced_ljac=None,
        mode=REJECT, oriented=True):
    """demczs_oracle.run (same arguments, same outputs) under the bounds rule `mode`, plus the census and the reflection
    outputs of tci_bounds_outputs for this cell: n_cross, oob_lo, oob_hi [n_pop, ld] (-1 at j >= P), n_left and n_refl
    [n_gen, n_pop], n_reflected [n_pop] and orient [n_pop, ld]. For the tests' own counts also flips [n_gen, n_pop], 1
    where an accepted proposal changed an orientation bit, and single_lo / single_hi, the coordinates that one reflection
    at the lower / upper wall brought back inside."""
    reflect = mode == REFLECT
    assert mode in (REJECT, REFLECT)
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
    nacc, noob, nnull, nreflected = (np.zeros(n_pop, np.int64) for _ in range(4))
    orient = np.zeros((n_pop, ld), np.uint8)
    ncross, ooblo, oobhi = (np.zeros((n_pop, ld), np.int64) for _ in range(3))
    for c in (ncross, ooblo, oobhi):
        c[:, P:] = -1
    nan = lambda: np.full((n_gen, n_pop), np.nan)  # noqa: E731
    logr, ljl, lj_own, lj_bound, s2_draw = nan(), nan(), nan(), nan(), nan()
    acc, oobl, snkl, flips = (np.zeros((n_gen, n_pop), np.uint8) for _ in range(4))
    nleft, nrefl = (np.zeros((n_gen, n_pop), np.int64) for _ in range(2))
    undecided = []
    single_lo = single_hi = 0
    kept = {k: [] for k in ("chain", "s2chain", "sschain", "prichain")}

    def keep():
        for k, a in zip(("chain", "s2chain", "sschain", "prichain"), (x, s2, ss, pri)):
            kept[k].append(a.copy())

    if thin > 0:
        keep()
    every = np.arange(n_pop)
    lo, up = np.asarray(lower, np.float64), np.asarray(upper, np.float64)
    for g in range(1, int(n_gen) + 1):
        jump = jump_every > 0 and g % jump_every == 0
        M = zso.archive_rows(g, m0, n_pop, append_every)
        a, c, e, jrand, snk, gs = zso.index_draws(seed, key, g, n_pop, M, P, p_snooker)
        snkl[g - 1] = snk
        t = x.copy()
        ot = orient.copy()
        flag = np.zeros(n_pop, np.int64)
        lj = np.zeros(n_pop)
        ii, si = np.flatnonzero(~snk), np.flatnonzero(snk)
        if len(ii):
            t[ii], ob, ot[ii], cross, below, above, refl, outside = parallel(x[ii], orient[ii], Z[a[ii]], Z[c[ii]], ii, jrand[ii], seed,
                                                                    key, g, P, lo, up, jitter, CR, gamma0, jump, reflect,
                                                                    oriented)
            flag[ii] = ob
            ncross[ii, :P] += cross
            ooblo[ii, :P] += below
            oobhi[ii, :P] += above
            nleft[g - 1, ii] = (below | above).sum(axis=1)
            nrefl[g - 1, ii] = refl.sum(axis=1)
            single_lo += int((refl & below & ~outside).sum())
            single_hi += int((refl & above & ~outside).sum())
        if len(si):
            t[si], flag[si], own, D, Dp = zso.snooker(x[si], Z[e[si]], Z[a[si]], Z[c[si]], gs[si], P, lo, up)
            lj[si] = own
            lj_own[g - 1, si] = own
            lj_bound[g - 1, si] = np.where(np.isfinite(own), zso.ljac_bound(P, D, Dp), np.nan)
            if forced_ljac is not None:
                lj[si] = np.where(flag[si] == 0, forced_ljac[g - 1, si], np.nan)
            moved = (flag[si] != 2)[:, None]            # a null move touches no counter
            with np.errstate(all="ignore"):
                below, above = moved & (t[si, :P] < lo[None, :P]), moved & (t[si, :P] > up[None, :P])
            ncross[si, :P] += moved
            ooblo[si, :P] += below
            oobhi[si, :P] += above
            nleft[g - 1, si] = np.where(flag[si] == 2, -1, (below | above).sum(axis=1))
        ljl[g - 1] = lj
        oobl[g - 1] = flag
        live = flag == 0
        nreflected += live & (nrefl[g - 1] > 0)
        ss_t = np.full(n_pop, np.inf)
        if live.any():   # a proposal rejected at the bounds, or a null move, is never evaluated
            ss_t[live] = np.asarray(ss_fn(t[live]), np.float64)
        pri_t = lpo.pri(t[:, :P], mu[:P], sig[:P])
        noob += flag == 1
        nnull += flag == 2
        w = dmo.rng_vec(seed, key, g, zso.P_ACCEPT, every)
        uu = dmo.u01_vec(w[0], w[1])
        with np.errstate(all="ignore"):
            fo = ss / s2 + pri
            fn = ss_t / s2 + pri_t
            lr = np.where(live, np.float64(-0.5) * (fn - fo) + lj, np.nan)
            ex = np.exp(lr)
            take = live & ((lr >= 0) | (uu < ex))      # a NaN logr fails both comparisons
            close = live & (lr < 0) & ~(np.abs(uu - ex) > zso.EXP_MARGIN * ex)
        logr[g - 1] = lr
        undecided += [(g, int(i)) for i in np.flatnonzero(close)]
        flips[g - 1] = take & (ot != orient).any(axis=1)
        x[take], ss[take], pri[take], orient[take] = t[take], ss_t[take], pri_t[take], ot[take]
        nacc += take
        acc[g - 1] = take
        if updatesigma:
            for i in range(n_pop):
                with np.errstate(all="ignore"):
                    gu = dmo.gamma_unit(seed, key, g, float(N), zso.P_SIGMA, i << 16)
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
               ljac=ljl, ljac_own=lj_own, ljac_bound=lj_bound, s2_draw=s2_draw, archive=Z, undecided=undecided,
               n_cross=ncross, oob_lo=ooblo, oob_hi=oobhi, n_left=nleft, n_refl=nrefl, n_reflected=nreflected,
               orient=orient, flips=flips, single_lo=single_lo, single_hi=single_hi)
    return out


# The flat-box validity case (tests/test_bounds_host.py on the restatement, tests/test_bounds_gpu.py on the device):
# P = 2, the box [0, 1]^2, a flat target, every in-box trial accepted. The archive's rows lie on the diagonal, so every
# difference is proportional to (1, 1), and it never grows (append_every above n_gen): the kernel is fixed. CR = 1 crosses
# both coordinates, so gamma = 2.38 / sqrt(4) = 1.19; the rows' diagonal coordinates are uniform on [0, SPREAD], so a step
# is +-1.19 times a difference of two of them: about 0.2 in size, a fifth of the box, and never beyond its width
# (1.19 * 0.5 + the jitter < 1), so no proposal needs a second reflection.
FLAT = dict(n_pop=128, m0=64, n_gen=1500, thin=1, n_burn=100, CR=1.0, jitter=0.03, spread=0.5, seed=3, pop_seed=5)


def flat_box(T=FLAT):
    """(pop0 [n_pop, 2], z0 [m0, 2], lower, upper, mu, sig, jitter) of the flat-box case: sig = Inf makes the prior 0."""
    rs = np.random.default_rng(T["pop_seed"])
    c = T["spread"] * rs.random(T["m0"])
    z0 = np.stack([c, c], axis=1)
    pop0 = rs.random((T["n_pop"], 2))
    return (pop0, z0, np.zeros(2), np.ones(2), np.full(2, 0.5), np.full(2, np.inf), np.full(2, T["jitter"]))


def flat_stats(chain):
    """The five statistics of chain [rows, n_pop, >= 2] against the uniform law on [0, 1]^2: the four quadrant masses
    (each 1/4) and E[(x1 - 1/2)(x2 - 1/2)] (0), each as |z| in Monte-Carlo standard errors, the statistic's own
    standard deviation under the uniform law over sqrt(ESS) with the ESS demc_oracle.ess_multi takes from the sample of
    that statistic. Returns (worst z, least ESS, the statistics' values)."""
    x1, x2 = chain[:, :, 0], chain[:, :, 1]
    hi1, hi2 = x1 > 0.5, x2 > 0.5
    series = [((hi1 == a) & (hi2 == b)).astype(np.float64) for a in (False, True) for b in (False, True)]
    want = [0.25] * 4 + [0.0]
    sd = [np.sqrt(0.25 * 0.75)] * 4 + [1.0 / 12.0]     # E[(x - 1/2)^2] = 1/12 per coordinate, independent
    series.append((x1 - 0.5) * (x2 - 0.5))
    zs, es, vals = [], [], []
    for s, w, d in zip(series, want, sd):
        e = dmo.ess_multi(s)
        es.append(e)
        vals.append(float(s.mean()))
        zs.append(abs(s.mean() - w) / (d / np.sqrt(e)))
    return max(zs), min(es), vals
