"""PSIS-LOO and stacking weights on the device (tci_loocheck / k_loocheck) against the numpy restatement
(tests/loocheck_oracle.py) applied to the rows ``Likelihood.forward(..., grid="interp")`` gives for the same theta, so
the simulated input is bit-identical.

Equalities: the NaN pattern and the scored mask, n_obs, khat = +Inf exactly where the restatement has it (a tail with
other members would not be degenerate at the same points), lppd_i (the bits of tci_fitcheck), n_khat_bad, and every
per-chain value recomputed from the returned pointwise vectors.

Tolerances: elpd_loo_i, p_loo_i, khat_i, the weights and elpd_stack pass through exp, log, log1p and expm1 and, for
khat, a weighted profile likelihood over up to 43 points; no useful a-priori bound came out. Each is compared with the
float64 restatement within FACTOR = 8 times the largest difference, over the call's points, between that restatement
and the same statements in numpy.longdouble (8: the device functions' 3-ulp limits against libm's sub-ulp). The
difference is measured on the call's own inputs, never from the device output, and printed; the values measured on the
test inputs are recorded in profiles/loocheck/tolerance.json."""
import json
import os

import numpy as np
import pytest

import loocheck_oracle as LO
from test_fitcheck_gpu import draw, sims, tame_s2

pytestmark = pytest.mark.gpu

FACTOR = 8.0     # profiles/loocheck/tolerance.json: "factor"
TOL_FIELDS = ("elpd_loo_i", "p_loo_i", "khat_i")
RECORD = os.environ.get("TCI_LOOCHECK_TOLERANCE_LOG")   # a file the measured differences are appended to


def record(name, diffs):
    print(f"{name}: max |float64 - longdouble| = {diffs}")
    if RECORD:
        with open(RECORD, "a") as f:
            f.write(json.dumps({"case": name, **{k: float(v) for k, v in diffs.items()}}) + "\n")


def lc_bytes(lc, k):
    fields = LO.POINTWISE + ("n_obs", "elpd_loo", "p_loo", "lppd", "khat_max", "n_khat_bad")
    return b"".join(getattr(lc, f)[k].tobytes() for f in fields)


def check(name, lk, theta, s2, cid, group=None, rows=None, **kw):
    """Likelihood.loocheck against the restatement; returns the LooCheck and the restatement's chains."""
    rows = rows or sims(lk, theta, cid)
    n_sel, S, _ = theta.shape
    thr = LO.default_threshold(S)
    refs, exs = [], []
    diffs = {f: 0.0 for f in TOL_FIELDS}
    for k, (m, p, y0, y1) in enumerate(rows):
        refs.append(LO.chain(m, p, y0, y1, s2[k]))
        exs.append(LO.chain(m, p, y0, y1, s2[k], exact=True))
        for f in TOL_FIELDS:
            with np.errstate(invalid="ignore"):
                d = np.abs(np.float64(exs[k][f] - refs[k][f].astype(np.longdouble)))
            both_inf = np.isinf(refs[k][f]) & (np.float64(exs[k][f]) == refs[k][f])
            d = d[~np.isnan(refs[k][f]) & ~both_inf]
            assert np.all(np.isfinite(d)), (k, f)                # the two paths agree on which tails are degenerate
            if d.size:
                diffs[f] = max(diffs[f], float(d.max()))
    record(name, diffs)
    # the inputs are chosen so that no khat of the restatement lies within the tolerance of the threshold: n_khat_bad
    # is then compared exactly for every chain. Checked on the CPU, before the device call.
    near = sum(int(np.sum(np.isfinite(r["khat_i"]) & (np.abs(r["khat_i"] - thr) <= FACTOR * diffs["khat_i"])))
               for r in refs)
    print(f"{name}: {near} points with khat within tolerance of the threshold")
    assert near == 0
    got = lk.loocheck(theta, s2, cid, group=group, **kw)
    fc = lk.fitcheck(theta, s2, cid)
    assert got.khat_threshold == thr and got.n_samples == S
    ld_out = int(lk.lengths[np.asarray(cid)].max())
    assert got.khat_i.shape == (n_sel, 2, ld_out)
    assert got.lppd_i.tobytes() == fc.lppd_i.tobytes()          # tci_fitcheck's bits
    for k, (m, p, y0, y1) in enumerate(rows):
        n, ref = len(y0), refs[k]
        scored = ~np.isnan(ref["khat_i"])
        assert np.array_equal(scored, np.isfinite(np.stack([y0, y1])) & np.stack(
            [np.all(np.isfinite(m), axis=0), np.all(np.isfinite(p), axis=0)]))
        for f in LO.POINTWISE:
            g = getattr(got, f)[k]
            assert np.all(np.isnan(g[:, n:])), (k, f)
            assert np.array_equal(np.isnan(g[:, :n]), ~scored), (k, f)
        assert int(got.n_obs[k]) == ref["n_obs"] == int(scored.sum())
        gk, rk = got.khat_i[k][:, :n], ref["khat_i"]
        assert np.array_equal(np.isposinf(gk), np.isposinf(rk)), k
        for f in TOL_FIELDS:
            g, r = getattr(got, f)[k][:, :n], ref[f]
            fin = scored & np.isfinite(r)
            err = np.abs(g[fin] - r[fin])
            if err.size:
                print(f"chain {k} {f}: max |gpu - f64| = {err.max():.3g}, tolerance = {FACTOR * diffs[f]:.3g}")
            assert np.all(err <= FACTOR * diffs[f]), (k, f, float(err.max()), FACTOR * diffs[f])
        assert int(got.n_khat_bad[k]) == ref["n_khat_bad"], k
        # the per-chain values are the host's sums over the pointwise vectors it returned
        mine = LO.per_chain({f: getattr(got, f)[k][:, :n] for f in LO.POINTWISE}, thr)
        assert mine["n_obs"] == int(got.n_obs[k]) and mine["n_khat_bad"] == int(got.n_khat_bad[k])
        for f in ("elpd_loo", "p_loo", "lppd", "khat_max"):
            assert np.array_equal(getattr(got, f)[k], np.float64(mine[f]), equal_nan=True), (k, f)
    if group is None:
        assert np.all(np.isnan(got.weight)) and got.elpd_stack.size == 0
    else:
        g = np.asarray(group)
        for gid in np.unique(g[g >= 0]):
            ks = np.flatnonzero(g == gid)
            e64 = np.stack([refs[k]["elpd_loo_i"].reshape(-1) for k in ks])
            eex = np.stack([exs[k]["elpd_loo_i"].reshape(-1) for k in ks])
            w, es, npts, _ = LO.stack(e64)
            wx, esx, nx, _ = LO.stack(eex)
            dw = float(np.max(np.abs(np.asarray(wx - w).astype(np.float64))))
            de = float(np.abs(np.asarray(esx - es).astype(np.float64)).max())
            record(f"{name} group {gid}", {"weight": dw, "elpd_stack": de})
            assert int(got.n_points[gid]) == npts == nx
            assert np.all(np.abs(got.weight[ks] - w) <= FACTOR * dw), (gid, got.weight[ks], w, dw)
            assert abs(got.elpd_stack[gid] - es) <= FACTOR * de, (gid, got.elpd_stack[gid], es, de)
            assert abs(got.weight[ks].sum() - 1.0) <= 1e-12
            # the host's iteration on the pointwise values it returned: the restatement on those gives its weights
            mine = LO.stack(np.stack([got.elpd_loo_i[k].reshape(-1) for k in ks]))
            assert np.all(np.abs(mine[0] - got.weight[ks]) <= 1e-9) and mine[2] == npts
        assert np.all(np.isnan(got.weight[g < 0]))
    return got, refs


@pytest.fixture(scope="module")
def lk(cells):
    from transcriptioncycleinference_amd import Likelihood

    with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as L:
        yield L


@pytest.fixture(scope="module")
def three(cells):
    order = np.argsort(cells.lengths, kind="stable")
    return np.array([order[0], order[len(order) // 2], order[-1]], np.int32)


@pytest.mark.parametrize("S", [32, 64, 65, 225, 500])
@pytest.mark.parametrize("n_sel", [1, 5])
def test_sample_counts(lk, three, S, n_sel):
    """The smallest S, the summation-segment edge on both sides, the switch between the two formulas for M and a typical
    value; one chain, and five chains (two cells with two chains each and one alone, grouped)."""
    rng = np.random.default_rng(1000 * n_sel + S)
    cid = three[[1]] if n_sel == 1 else three[[1, 0, 1, 2, 0]]
    group = None if n_sel == 1 else np.array([0, 2, 0, -1, 2], np.int32)
    theta = draw(rng, lk.lengths, cid, S)
    rows = sims(lk, theta, cid)
    got, _ = check(f"S{S}_n{n_sel}", lk, theta, tame_s2(rows, rng, S), cid, group=group, rows=rows)
    assert np.all(got.n_obs > 0) and np.all(np.isfinite(got.elpd_loo))
    if n_sel == 5:
        assert got.n_points[1] == 0 and np.isnan(got.elpd_stack[1])       # an empty group


def test_the_cap(lk, three):
    """S = 4096: the largest tail (M = 192, 120 KiB of LDS for the heap), one cell."""
    S = 4096
    rng = np.random.default_rng(4096)
    cid = three[[0]]
    theta = draw(rng, lk.lengths, cid, S)
    rows = sims(lk, theta, cid)
    check("S4096", lk, theta, tame_s2(rows, rng, S), cid, group=np.zeros(1, np.int32), rows=rows)


def test_ragged_table_shortest_and_longest():
    """The cells of 2 and 258 points of the rpl8 context of tests/ragged_cases.py, and two values of scratch_bytes, one
    of which forces a chunk per chain: the same bits."""
    import ragged_cases as RC
    from transcriptioncycleinference_amd import Likelihood, from_lists

    k = RC.case("rpl8", "builtin")
    lengths = [len(c[0]) for c in k.cl]
    cid = np.array([next(c for c in range(len(lengths)) if lengths[c] == n and not k.twin[c]) for n in (2, 258, 2)],
                   np.int32)
    S = 65
    rng = np.random.default_rng(259)
    with Likelihood(from_lists(k.cl), "P2P-MS2v5-LacZ-PP7v4") as L:
        theta = draw(rng, L.lengths, cid, S, ld=k.ld)
        rows = sims(L, theta, cid)
        s2 = tame_s2(rows, rng, S)
        group = np.array([0, -1, 0], np.int32)
        whole, _ = check("ragged", L, theta, s2, cid, group=group, rows=rows)
        per_chain = 2 * S * 258 * 8
        for cap in (per_chain, 2 * per_chain + 8):
            part = L.loocheck(theta, s2, cid, group=group, scratch_bytes=cap)
            for i in range(3):
                assert lc_bytes(part, i) == lc_bytes(whole, i)
            assert part.weight.tobytes() == whole.weight.tobytes()
            assert part.elpd_stack.tobytes() == whole.elpd_stack.tobytes()
    assert whole.khat_i.shape == (3, 2, 258) and np.all(np.isnan(whole.khat_i[0, :, 2:]))


def test_missing_data():
    """NaN data scattered in one dye and a dye that is all NaN: unscored points, and groups whose common points are
    fewer than either chain's."""
    from transcriptioncycleinference_amd import Likelihood, from_lists
    from transcriptioncycleinference_amd.data import synthetic_times

    rng = np.random.default_rng(41)
    cl = []
    for n in (70, 131):
        cl.append([synthetic_times(rng, n), rng.normal(3, 2, n), rng.normal(6, 3, n)])
    cl[0][1][rng.random(70) < 0.3] = np.nan
    cl[0][1][[0, 63, 64, 69]] = np.nan
    cl[1][2][:] = np.nan
    cid = np.array([0, 1, 0], np.int32)
    S = 70
    with Likelihood(from_lists([tuple(c) for c in cl]), "P2P-MS2v5-LacZ-PP7v4") as L:
        theta = draw(rng, L.lengths, cid, S)
        rows = sims(L, theta, cid)
        got, _ = check("missing", L, theta, tame_s2(rows, rng, S), cid, group=np.array([0, 1, 0], np.int32), rows=rows)
    assert got.n_obs[0] == 70 + int(np.isfinite(cl[0][1]).sum()) == got.n_points[0] and got.n_obs[1] == 131
    assert got.weight[1] == 1.0 and got.n_iter[1] == 0


def test_ties_across_the_cut(lk, chain):
    """Rows of a short real chain, repeated: equal ratios on both sides of the cut, so membership and rank go by the
    sample index."""
    cells_in = np.asarray(chain["cell_id"])
    c = int(np.bincount(cells_in).argmax())
    mine = np.flatnonzero(cells_in == c)
    d = min(len(mine), 32)
    S = 225
    pick = mine[np.arange(S) % d]
    theta = np.stack([chain["rows"][i] for i in pick])[None]
    s2 = np.full((1, S), float(np.median(np.asarray(chain["s2"])[mine])))   # one sigma2: equal rows give equal ratios
    cid = np.array([c], np.int32)
    rows = sims(lk, theta, cid)
    M, _ = LO.tail_count(S)
    straddle = 0
    for f, y in ((rows[0][0], rows[0][2]), (rows[0][1], rows[0][3])):
        ll, scored = LO.log_lik(f, y, s2[0])
        lr, idx, cut = LO.select_tail(ll)
        first = np.take_along_axis(lr, idx[:1], axis=0)[0]
        straddle += int(np.sum(scored & (first == cut)))
    assert straddle >= 10                                       # the property this case exists for
    got, refs = check("ties", lk, theta, s2, cid, rows=rows)
    assert np.isfinite(refs[0]["khat_i"]).sum() >= 10           # ranks inside tied groups reach the smoothed values


def test_position_and_grouping_do_not_change_the_bits(lk, three):
    S = 130
    rng = np.random.default_rng(43)
    cid = three[[0, 0, 1, 0, 1]]
    theta = draw(rng, lk.lengths, cid, S)
    s2 = tame_s2(sims(lk, theta, cid), rng, S)
    a = lk.loocheck(theta, s2, cid, group=np.array([0, 0, 1, 0, 1], np.int32))
    order = [2, 0, 4, 1, 3]                                      # the members of each group keep their order
    wide = np.zeros((5, S, theta.shape[2] + 9))
    wide[:, :, :theta.shape[2]] = theta
    b = lk.loocheck(wide[order], s2[order], cid[order], group=np.array([3, 1, 3, 1, 1], np.int32))
    for i, k in enumerate(order):
        assert lc_bytes(b, i) == lc_bytes(a, k)
        assert b.weight[i].tobytes() == a.weight[k].tobytes()
    assert b.elpd_stack[[1, 3]].tobytes() == a.elpd_stack[[0, 1]].tobytes()
    assert b.n_iter[[1, 3]].tolist() == a.n_iter[[0, 1]].tolist() and b.n_points[[0, 2]].tolist() == [0, 0]
    alone = lk.loocheck(theta[:1], s2[:1], cid[:1])
    n0 = int(lk.lengths[cid[0]])
    for f in LO.POINTWISE:
        assert getattr(alone, f)[0][:, :n0].tobytes() == getattr(a, f)[0][:, :n0].tobytes(), f
    two = lk.loocheck(theta[[0, 0]], s2[[0, 0]], cid[[0, 0]], group=np.zeros(2, np.int32))
    assert two.weight.tobytes() == np.array([0.5, 0.5]).tobytes()


def test_argument_checks(lk, three):
    from transcriptioncycleinference_amd import _lib

    rng = np.random.default_rng(44)
    theta = draw(rng, lk.lengths, three[:2], 40)
    s2 = np.ones((2, 40))
    with pytest.raises(ValueError, match="32"):
        lk.loocheck(theta[:, :31], s2[:, :31], three[:2])
    with pytest.raises(ValueError, match="one cell"):
        lk.loocheck(theta, s2, three[:2], group=np.zeros(2, np.int32))
    out = _lib.tci_loocheck_outputs()
    P = lambda a, t=_lib._dp: _lib.ptr(a, t)  # noqa: E731
    cid = np.ascontiguousarray(three[:2], np.int32)
    for S, grp, ng, code in ((31, None, 0, _lib.TCI_EINVAL), (40, np.zeros(2, np.int32), 1, _lib.TCI_EINVAL),
                             (40, np.array([0, 1], np.int32), 1, _lib.TCI_ERANGE)):
        opt = _lib.tci_loocheck_options(0, ng, 0.0, 5000, 1e-12)
        rc = lk._lib.tci_loocheck(lk._h, opt, P(theta), theta.shape[2], P(s2), P(cid, _lib._i32p), P(grp, _lib._i32p), 2,
                                  S, int(lk.lengths[cid].max()), out)
        assert rc == code, (S, rc)


def test_through_fit(lk, cells):
    """fit(..., replicates=4, stack=64): MCMCresults are those of the fit without stack, and every field of MCMCstack
    equals Likelihood.loocheck on the same rows of all four replicates, taken from a sampler run with fit's inputs."""
    from transcriptioncycleinference_amd import mcmc

    ids, M, n_steps, n_burn, thin, seed = [0, 150, 298], 4, 1200, 600, 5, 3
    K = len(ids)
    kw = dict(n_steps=n_steps, n_burn=n_burn, seed=seed, thin=thin, cells=ids, replicates=M)
    plain = mcmc.fit(lk, **kw)
    fit = mcmc.fit(lk, stack=64, **kw)
    assert plain.MCMCstack is None and len(fit.MCMCstack) == K
    for a, b in zip(plain.MCMCresults, fit.MCMCresults):
        for f in mcmc.RESULT_FIELDS:
            assert np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes(), f
    # the sampler run fit makes (mcmc.fit's own lines), keeping every replicate's rows
    plan = mcmc.plan_fit(cells, ids, seed, replicates=M)
    o = mcmc.DramOptions()
    o.n_steps, o.burnintime, o.stats_from, o.thin = n_steps, n_burn, n_burn, thin
    o.seed = seed * 1000003 + 20201028
    res = mcmc.dram_run(lk, np.tile(np.array(ids, np.int32), M), plan.x0, plan.lower, plan.upper, plan.prior_mu,
                        plan.prior_sig, plan.qcov_diag, 1.0, o,
                        chain_keys=mcmc.replicate_keys(np.array(ids, np.int64), M))
    kept = res.chain[1 + thin * np.arange(res.chain.shape[0]) >= n_burn]
    rows = kept.shape[0]
    idx = mcmc.predict_rows(rows, 64)
    assert rows == 120 and len(idx) == 64 and len(np.unique(idx)) == 64
    for k, c in enumerate(ids):                                   # replicate 0 is the chain the result file keeps
        n = int(cells.lengths[c])
        assert np.array_equal(kept[:, k, :7 + n], mcmc.chain_theta(fit.MCMCchain[k], n, np.arange(rows)))
        assert np.array_equal(res.s2chain[-rows:, k], fit.MCMCchain[k]["s2chain"][-rows:])
    # chain r * K + k is replicate r of cell k; one call, with the cells' replicates as groups in another numbering
    theta = np.ascontiguousarray(np.transpose(kept[idx], (1, 0, 2)))
    s2 = np.ascontiguousarray(res.s2chain[-rows:][idx].T)
    assert len({s2[i].tobytes() for i in range(M * K)}) == M * K   # a wrong pairing of s2 rows would show
    want = lk.loocheck(theta, s2, np.tile(np.array(ids, np.int32), M), group=np.tile(np.array([2, 0, 1], np.int32), M))
    for k, c in enumerate(ids):
        n = int(cells.lengths[c])
        e = fit.MCMCstack[k]
        ch = [r * K + k for r in range(M)]
        for f in ("elpd_loo", "p_loo", "khat_max", "n_khat_bad"):
            assert e[f].shape == (M,) and e[f].tobytes() == getattr(want, f)[ch].tobytes(), f
        assert e["weights"].shape == (M,) and e["weights"].tobytes() == want.weight[ch].tobytes()
        assert np.float64(e["elpd_stack"]).tobytes() == want.elpd_stack[[2, 0, 1][k]].tobytes()
        assert e["elpd_loo_i"].tobytes() == np.ascontiguousarray(want.elpd_loo_i[k][:, :n]).tobytes()
        assert e["khat_i"].tobytes() == np.ascontiguousarray(want.khat_i[k][:, :n]).tobytes()
        assert abs(e["weights"].sum() - 1) < 1e-12 and np.all(e["weights"] >= 0)
        assert e["cell_index"] == c + 1 and e["n_samples"] == 64
        assert np.array_equal(e["stacked_mean"], e["weights"] @ res.mean[ch, :7 + n])
        assert np.array_equal(res.mean[ch, :7 + n], fit.MCMCrhat[k]["mean_rep"][:, :7 + n])
        assert len({v.tobytes() for v in e["elpd_loo"]}) == M     # the replicates differ: a wrong stride would show
    solo = mcmc.fit(lk, stack=64, **{**kw, "replicates": 1})
    assert [e["weights"].tolist() for e in solo.MCMCstack] == [[1.0]] * K
    for a, b in zip(solo.MCMCstack, fit.MCMCstack):               # replicate 0 alone: the same chain, the same LOO
        assert a["elpd_loo"][0] == b["elpd_loo"][0] and a["elpd_loo_i"].tobytes() == b["elpd_loo_i"].tobytes()
