"""The log-posterior trace on the device (tci_chainlp / tci_chainlp.hip) against the numpy restatement
(tests/chainlp_oracle.py) and the entries it is defined by: ss is Likelihood.ss_batch on the same rows, theta_mean is
Likelihood.chaincov's mean, ss_hat is ss_batch of theta_mean, all bit for bit; pri and every reduced value equal the
restatement applied to the returned traces bit for bit. dev, lp and d_hat go through log: within twice the header's
bound of the float64 restatement (both sides round) and within the bound of the long-double path, and every bound used
is asserted to be at most 1e-10 max(1, |value|), so a lax bound cannot hide a failure. sigma2 is chosen for that
(tame_s2: ss / s2 stays near the observation count)."""
import numpy as np
import pytest

import chainlp_oracle as O
import variant_rows as VR

pytestmark = pytest.mark.gpu

CAP = 1e-10
SMALL = (10, 57, 58, 123, 30)      # P = 17, 64, 65, 130, 37: the lane edges of the prior sum
FIELDS = O.SCALARS + ("best_row", "theta_best", "theta_mean")


def synthetic(lengths, seed):
    from transcriptioncycleinference_amd import from_lists

    rng = np.random.default_rng(seed)
    cl = []
    for n in lengths:
        cl += VR.synthetic_cell_list(rng, n, n_cells=1)
    return from_lists(cl)


@pytest.fixture(scope="module")
def lk():
    from transcriptioncycleinference_amd import Likelihood

    with Likelihood(synthetic(SMALL, 41), "P2P-MS2v5-LacZ-PP7v4", device=0) as L:
        yield L


@pytest.fixture(scope="module")
def lk_long():
    from transcriptioncycleinference_amd import Likelihood

    with Likelihood(synthetic((600,), 42), "P2P-MS2v5-LacZ-PP7v4", device=0) as L:
        assert L.info["rows_per_lane"] == 0   # the long-cell kernel
        yield L


def make_chain(rng, lengths, cid, rows, ld=None, pad=np.nan):
    """chain [rows, C, ld] of draw_x0 rows inside the reference's bounds, duplicated in runs of 1 to 4 as a real chain
    is (rejected proposals repeat the row); the padding past a chain's P holds `pad`."""
    from transcriptioncycleinference_amd.data import draw_x0

    P = 7 + lengths[np.asarray(cid)]
    ld = ld or int(P.max())
    chain = np.full((rows, len(cid), ld), pad)
    for c in range(len(cid)):
        t = 0
        while t < rows:
            run = int(rng.integers(1, 5))
            chain[t:t + run, c, :P[c]] = draw_x0(rng, int(lengths[cid[c]]))
            t += run
    return chain


def priors(rng, P, ld):
    """mu finite, sig a mix of +Inf and finite on both the scalars and the rates; padding NaN (never read)."""
    C = len(P)
    mu, sig = np.full((C, ld), np.nan), np.full((C, ld), np.nan)
    for c in range(C):
        mu[c, :P[c]] = rng.normal(0.0, 1.0, P[c])
        sig[c, :P[c]] = np.where(rng.random(P[c]) < 0.4, np.inf, rng.uniform(0.5, 50.0, P[c]))
        sig[c, 0], sig[c, 7] = np.inf, 50.0
    return mu, sig


def tame_s2(ss, nobs, rng):
    """sigma2 [rows, C] with ss / s2 <= nobs: (the chain's largest finite ss / nobs) times U(1, 3)."""
    big = np.array([np.max(col[np.isfinite(col)], initial=1.0) for col in ss.T])
    return (big / nobs)[None, :] * rng.uniform(1.0, 3.0, ss.shape)


def ss_rows(lk, chain, cid):
    rows, C, ld = chain.shape
    return lk.ss_batch(chain.reshape(rows * C, ld), np.tile(np.asarray(cid, np.int32), rows)).reshape(rows, C)


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def check(lk, chain, s2, cid, mu, sig, ss_ref=None):
    """Likelihood.chainlp against its definition; returns the ChainLp."""
    rows, C, ld = chain.shape
    cid = np.asarray(cid, np.int32)
    P = (7 + lk.lengths[cid]).astype(int)
    nobs = (2 * lk.lengths[cid]).astype(np.float64)
    got = lk.chainlp(chain, s2, cid, mu, sig)
    assert got.n_rows == rows and got.ss.shape == (rows, C) and got.theta_best.shape == (C, ld)
    assert same(got.ss, ss_rows(lk, chain, cid) if ss_ref is None else ss_ref), "ss is not ss_batch's"
    pri, dev, lp = O.traces(chain, s2, got.ss, P, nobs, mu, sig)
    assert same(got.pri, pri), "pri"
    dev_x = O.dev(got.ss, s2, nobs[None, :], exact=True)
    lp_x = O.lp(dev_x, got.pri, exact=True)
    e_dev, e_lp = O.bounds(got.ss, s2, nobs[None, :], dev, lp)
    for name, g, r64, rx, b in (("dev", got.dev, dev, dev_x, e_dev), ("lp", got.lp, lp, lp_x, e_lp)):
        assert np.array_equal(np.isnan(g), np.isnan(r64)), name
        ok = np.isfinite(r64)
        e64 = np.abs(g[ok] - r64[ok])
        eex = np.abs(g[ok].astype(O.LD) - rx[ok]).astype(np.float64)
        if ok.any():
            print(f"{name}: max |gpu - f64| / bound = {np.max(e64 / b[ok]):.3g}, max |gpu - exact| / bound = "
                  f"{np.max(eex / b[ok]):.3g}, max bound = {np.max(b[ok]):.3g}")
        assert np.all(b[ok] <= CAP * np.maximum(1.0, np.abs(r64[ok]))), name
        assert np.all(e64 <= 2.0 * b[ok]) and np.all(eex <= b[ok]), name
    # the means are tci_chaincov's, the SS of the mean row the likelihood kernel's
    good = got.best_row >= 0
    tm = lk.chaincov(chain, npar=P).mean if rows >= 2 else np.stack(
        [np.concatenate([O.col_mean(chain[:, c, :P[c]]), np.full(ld - P[c], np.nan)]) for c in range(C)])
    sm = O.col_mean(s2)
    assert same(got.theta_mean[good], tm[good]) and same(got.s2_mean[good], sm[good])
    ss_hat = np.full(C, np.nan)
    if good.any():
        ss_hat[good] = lk.ss_batch(got.theta_mean[good], cid[good])
    # every reduced value is exact arithmetic on the returned traces
    ref = O.reduce({f: getattr(got, f) for f in ("ss", "pri", "dev", "lp")}, s2, chain, P, nobs, tm, sm, ss_hat)
    assert same(good, ref["best_row"] >= 0)
    for f in FIELDS:
        if f not in ("d_hat", "p_d", "dic"):
            assert same(getattr(got, f), ref[f]), f
    for c in np.nonzero(good)[0]:
        assert same(got.theta_best[c, :P[c]], chain[got.best_row[c], c, :P[c]])
        assert np.all(got.lp[:got.best_row[c], c] < got.lp_best[c]) and np.all(got.lp[:, c] <= got.lp_best[c])
    # d_hat goes through log; p_d and dic are exact on the device's d_hat
    dh_x = O.dev(got.ss_hat, got.s2_mean, nobs, exact=True)
    b = O.bounds(got.ss_hat, got.s2_mean, nobs, ref["d_hat"], 0.0)[0]
    g = good & np.isfinite(ref["d_hat"])
    assert same(np.isnan(got.d_hat), np.isnan(ref["d_hat"]))
    assert np.all(b[g] <= CAP * np.maximum(1.0, np.abs(ref["d_hat"][g])))
    assert np.all(np.abs(got.d_hat[g] - ref["d_hat"][g]) <= 2.0 * b[g])
    assert np.all(np.abs(got.d_hat[g].astype(O.LD) - dh_x[g]).astype(np.float64) <= b[g])
    with np.errstate(invalid="ignore"):
        assert same(got.p_d, got.dev_mean - got.d_hat) and same(got.dic, got.dev_mean + got.p_d)
    return got


def lp_bytes(g, c):
    return b"".join(np.ascontiguousarray(getattr(g, f)[:, c]).tobytes() for f in ("ss", "pri", "dev", "lp")) + b"".join(
        np.ascontiguousarray(getattr(g, f)[c]).tobytes() for f in O.SCALARS + ("best_row",))


def case(lk, seed, cid, rows, ld=None):
    rng = np.random.default_rng(seed)
    cid = np.asarray(cid, np.int32)
    chain = make_chain(rng, lk.lengths, cid, rows, ld)
    P = (7 + lk.lengths[cid]).astype(int)
    mu, sig = priors(rng, P, chain.shape[2])
    ss = ss_rows(lk, chain, cid)
    s2 = tame_s2(ss, 2.0 * lk.lengths[cid], rng)
    return chain, s2, cid, mu, sig, ss


@pytest.mark.parametrize("rows", [1, 2, 255, 256, 257, 513])
def test_segment_edges(lk, rows):
    """Three chains on cells of P = 64, 65 and 130 (the lane edges), ragged: ld = 130 with NaN padding."""
    chain, s2, cid, mu, sig, ss = case(lk, 100 + rows, [1, 2, 3], rows)
    got = check(lk, chain, s2, cid, mu, sig, ss)
    assert np.all(got.best_row >= 0) and np.all(np.isfinite(got.dic))
    assert np.all(np.isnan(got.dev_var)) if rows == 1 else np.all(got.dev_var >= 0)
    assert np.all(np.isnan(got.theta_best[0, 64:])) and np.all(np.isnan(got.theta_mean[1, 65:]))


@pytest.mark.parametrize("cid", [[0], [3, 1, 3], [4, 0, 2, 2, 1]])
def test_chain_counts_and_shared_cells(lk, cid):
    chain, s2, cid, mu, sig, ss = case(lk, 200 + len(cid), cid, 300, ld=140)
    check(lk, chain, s2, cid, mu, sig, ss)


def test_long_cell_kernel(lk_long):
    chain, s2, cid, mu, sig, ss = case(lk_long, 300, [0], 3)
    got = check(lk_long, chain, s2, cid, mu, sig, ss)
    assert got.best_row[0] >= 0


def test_duplicate_rows_give_the_first(lk):
    """The best row copied (theta and sigma2) to rows before and after it: the same lp bits, the least row wins."""
    chain, s2, cid, mu, sig, _ = case(lk, 400, [1, 4], 40)
    got = check(lk, chain, s2, cid, mu, sig)
    b = int(got.best_row[0])
    rows = sorted({2, 9, 33, 39} - {b})
    chain[rows, 0], s2[rows, 0] = chain[b, 0], s2[b, 0]
    dup = check(lk, chain, s2, cid, mu, sig)
    assert len({dup.lp[t, 0].tobytes() for t in rows + [b]}) == 1 and dup.lp_best[0] == got.lp_best[0]
    assert dup.best_row[0] == min(rows[0], b) and same(dup.theta_best[0], got.theta_best[0])
    assert lp_bytes(dup, 1) == lp_bytes(got, 1)


def test_a_nan_poisons_its_chain_alone(lk):
    chain, s2, cid, mu, sig, _ = case(lk, 500, [2, 3, 0], 260)
    clean = check(lk, chain, s2, cid, mu, sig)
    for what in ("theta", "s2"):
        ch, s = chain.copy(), s2.copy()
        if what == "theta":
            ch[258, 1, 3] = np.nan
        else:
            s[4, 1] = -1.0             # log of a negative number
        got = check(lk, ch, s, cid, mu, sig)
        assert got.best_row.tolist()[1] == -1 and all(np.isnan(getattr(got, f)[1]) for f in O.SCALARS)
        assert np.all(np.isnan(got.theta_best[1])) and np.all(np.isnan(got.theta_mean[1]))
        for c in (0, 2):
            assert lp_bytes(got, c) == lp_bytes(clean, c)
            assert same(got.theta_best[c], clean.theta_best[c]) and same(got.theta_mean[c], clean.theta_mean[c])


def test_bits_do_not_depend_on_the_layout(lk):
    chain, s2, cid, mu, sig, _ = case(lk, 600, [1, 3, 0, 2], 300)
    base = lk.chainlp(chain, s2, cid, mu, sig)
    perm = np.array([2, 0, 3, 1])
    g = lk.chainlp(chain[:, perm], s2[:, perm], cid[perm], mu[perm], sig[perm])         # permuted
    for k, c in enumerate(perm):
        assert lp_bytes(g, k) == lp_bytes(base, c) and same(g.theta_best[k], base.theta_best[c])
    ld2 = chain.shape[2] + 9                                                              # a larger ld
    wide = lambda a, fill: np.concatenate([a, np.full(a.shape[:-1] + (9,), fill)], axis=-1)  # noqa: E731
    g = lk.chainlp(wide(chain, -7.0), s2, cid, wide(mu, np.nan), wide(sig, -1.0))
    assert g.theta_best.shape == (4, ld2)
    for c in range(4):
        assert lp_bytes(g, c) == lp_bytes(base, c) and same(g.theta_best[c, :-9], base.theta_best[c])
    extra, s2e, cide, mue, sige, _ = case(lk, 601, [4, 4, 1], 300, ld=chain.shape[2])    # unrelated chains around
    g = lk.chainlp(np.concatenate([extra[:, :2], chain, extra[:, 2:]], axis=1),
                   np.concatenate([s2e[:, :2], s2, s2e[:, 2:]], axis=1), np.concatenate([cide[:2], cid, cide[2:]]),
                   np.concatenate([mue[:2], mu, mue[2:]]), np.concatenate([sige[:2], sig, sige[2:]]))
    for c in range(4):
        assert lp_bytes(g, 2 + c) == lp_bytes(base, c) and same(g.theta_mean[2 + c], base.theta_mean[c])


def test_arguments_are_checked_by_the_library(lk):
    from transcriptioncycleinference_amd import _lib

    chain, s2, cid, mu, sig, _ = case(lk, 700, [0, 1], 4)

    def code(**kw):
        a = dict(chain=chain, s2chain=s2, cell_id=cid, prior_mu=mu, prior_sig=sig)
        a.update(kw)
        with pytest.raises(_lib.TciError) as e:
            lk.chainlp(**a)
        return e.value.code, str(e.value)

    bad = mu.copy()
    bad[1, 5] = np.inf
    c, msg = code(prior_mu=bad)
    assert c == _lib.TCI_EINVAL and "chain 1, index 5" in msg
    for v in (np.nan, 0.0, -2.0):
        bad = sig.copy()
        bad[0, 9] = v
        c, msg = code(prior_sig=bad)
        assert c == _lib.TCI_EINVAL and "chain 0, index 9" in msg
    assert code(cell_id=np.array([0, 99], np.int32))[0] == _lib.TCI_ERANGE
    assert code(chain=chain[:, :, :30], prior_mu=mu[:, :30], prior_sig=sig[:, :30])[0] == _lib.TCI_ERANGE   # ld < 7 + N


@pytest.fixture(scope="module")
def tlk(cells):
    from transcriptioncycleinference_amd import Likelihood

    with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as L:
        yield L


@pytest.mark.parametrize("engine", ["fused", "batched", "walk"])
def test_the_run_path_equals_the_host_entry(tlk, engine):
    """tci_dram_run_lp on three TestData cells: the bits of tci_chainlp on the returned chain; the SS of
    the last kept row is ssfun of the final state."""
    from transcriptioncycleinference_amd import mcmc

    order = np.argsort(tlk.lengths, kind="stable")
    ids = [int(order[0]), int(order[len(order) // 2]), int(order[-1])]
    plan = mcmc.plan_fit(tlk.cells, ids, seed=5)
    o = mcmc.DramOptions(n_steps=300, burnintime=100, adaptint=50, stats_from=41, thin=1, seed=9, engine=engine)
    cid = np.array(ids, np.int32)
    res = mcmc.dram_run(tlk, cid, plan.x0, plan.lower, plan.upper, plan.prior_mu, plan.prior_sig, plan.qcov_diag, 1.0, o,
                        logpost=True)
    assert res.lp.n_rows == 260 and res.lp.ss.shape == (260, 3)
    want = tlk.chainlp(res.chain[40:], res.s2chain[40:], cid, plan.prior_mu, plan.prior_sig)
    for c in range(3):
        assert lp_bytes(res.lp, c) == lp_bytes(want, c)
    assert same(res.lp.theta_best, want.theta_best) and same(res.lp.theta_mean, want.theta_mean)
    for c, cell in enumerate(ids):
        P = 7 + int(tlk.lengths[cell])
        assert res.lp.ss[-1, c] == tlk.ssfun(res.final_theta[c, :P], cell)
    quiet = mcmc.dram_run(tlk, cid, plan.x0, plan.lower, plan.upper, plan.prior_mu, plan.prior_sig, plan.qcov_diag, 1.0, o,
                          logpost=True, want_chain=False, stats=True)       # with another reduction, no host chain
    assert quiet.chain is None and all(lp_bytes(quiet.lp, c) == lp_bytes(want, c) for c in range(3))
    alone = mcmc.dram_run(tlk, cid, plan.x0, plan.lower, plan.upper, plan.prior_mu, plan.prior_sig, plan.qcov_diag, 1.0, o,
                          want_chain=False, stats=True)
    assert quiet.stats.n_rows == alone.stats.n_rows == 260
    for f in ("mcerr", "tau", "tau_window", "geweke_z", "geweke_p", "s2_mcerr", "s2_tau", "s2_geweke_p"):
        assert same(getattr(quiet.stats, f), getattr(alone.stats, f)), f
    from transcriptioncycleinference_amd import _lib
    for bad in (mcmc.DramOptions(n_steps=50, thin=0), mcmc.DramOptions(n_steps=50, thin=1, stats_from=51)):
        with pytest.raises(_lib.TciError) as e:      # no kept row for the trace
            mcmc.dram_run(tlk, cid, plan.x0, plan.lower, plan.upper, plan.prior_mu, plan.prior_sig, plan.qcov_diag, 1.0,
                          bad, logpost=True)
        assert e.value.code == _lib.TCI_EINVAL and "tci_dram_run_lp" in str(e.value)
    sig = plan.prior_sig.copy()
    sig[1, 8] = -1.0                                 # a prior the trace cannot use is refused before the run
    with pytest.raises(_lib.TciError) as e:
        mcmc.dram_run(tlk, cid, plan.x0, plan.lower, plan.upper, plan.prior_mu, sig, plan.qcov_diag, 1.0, o, logpost=True)
    assert e.value.code == _lib.TCI_EINVAL and "chain 1, index 8" in str(e.value)


def test_fit_with_replicates_carries_the_lp_diagnostics(tlk):
    from transcriptioncycleinference_amd import mcmc

    order = np.argsort(tlk.lengths, kind="stable")
    ids = [int(order[0]), int(order[1])]
    fr = mcmc.fit(tlk, n_steps=240, n_burn=41, thin=1, seed=3, cells=ids, replicates=2, logpost=True)
    assert len(fr.MCMClp) == 2
    for k, e in enumerate(fr.MCMClp):
        assert set(e) == set(mcmc.LP_FIELDS + mcmc.LP_GROUP_FIELDS) and e["cell_index"] == ids[k] + 1
        assert e["lp"].shape == (2, 200) and e["n_chains"] == 2 and e["best_dR"].shape == (2, int(tlk.lengths[ids[k]]))
        col = np.ascontiguousarray(e["lp"].T[:, :, None])
        cr, ce = tlk.chainrhat(col), tlk.chainess(col)
        assert e["lp_rhat"] == cr.rhat[0, 0] and e["lp_rhat_split"] == cr.rhat_split[0, 0]
        assert e["lp_ess"] == ce.ess[0, 0] and e["lp_mcse"] == ce.mcse[0, 0]
        assert e["ss_gap"] == np.max(e["ss_mean"]) - np.min(e["ss_mean"]) and e["best_replicate"] == int(np.argmax(e["lp_best"]))
        assert np.array_equal(e["ss"][0], fr.MCMClp[k]["ss"][0]) and np.all(e["ss_min"] <= e["ss_mean"])
    one = mcmc.fit(tlk, n_steps=240, n_burn=41, thin=1, seed=3, cells=ids, logpost=True)     # replicate 0 is the one-chain fit
    for k, e in enumerate(one.MCMClp):
        assert isinstance(e["dic"], float) and e["dic"] == fr.MCMClp[k]["dic"][0] and same(e["lp"], fr.MCMClp[k]["lp"][0])


def test_the_sharded_fit_gathers_the_entries(tlk):
    """parallel.fit_sharded(logpost=True) without a process group (the one-rank case): the gathered MCMClp, traces
    included, equals fit's."""
    from transcriptioncycleinference_amd import mcmc, parallel

    kw = dict(n_steps=120, n_burn=21, thin=2, seed=4, logpost=True)
    for M in (1, 2):
        sh = parallel.fit_sharded(tlk, replicates=M, **kw)
        ids = [int(c) for c in sh.cell_index[[0, 5, -1]]]
        pmax = 7 + int(tlk.lengths.max())      # the adaptation kernel the whole fit picks (DramOptions.adapt_pmax)
        one = mcmc.fit(tlk, cells=ids, replicates=M, opts=mcmc.DramOptions(adapt_pmax=pmax), **kw)
        assert len(sh.MCMClp) == tlk.cells.n_cells and sh.local.MCMClp is not None
        for e in one.MCMClp:
            g = sh.MCMClp[e["cell_index"] - 1]
            assert set(g) == set(e) and g["n_rows"] == 50
            for f in e:
                assert same(g[f], e[f]) and np.shape(g[f]) == np.shape(e[f]), f
