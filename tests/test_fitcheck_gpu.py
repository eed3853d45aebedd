"""Posterior predictive fit checks on the device (tci_fitcheck / k_fitcheck) against the numpy restatement
(tests/fitcheck_oracle.py) applied to the rows ``Likelihood.forward(..., grid="interp")`` gives for the same theta, so
the simulated input is bit-identical.

Equalities: resid, zbar and z2 (+, -, x and / in a stated order), the NaN pattern, n_obs, and every per-cell value
recomputed from the returned pointwise vectors. lppd, p_waic and pit go through exp, log and erfc: they lie within
twice the header's bound of the float64 restatement (both sides round) and within the bound of the long-double path.
Every test also asserts that the bound it used is at most 1e-10 * max(1, |value|), the project's parity tolerance, so
a lax bound cannot hide a failure. sigma2 is chosen for that (tame_s2: |z| <= 30): with Z2 <= 900 and S <= 4096 the
header's D is below 1.5e-11, so p_waic's bound, about 2 D sqrt(p_waic), stays under the cap whatever p_waic is."""
import numpy as np
import pytest

import fitcheck_oracle as FO

pytestmark = pytest.mark.gpu

LEVELS = (0.5, 0.8, 0.95)
CAP = 1e-10


def sims(lk, theta, cid):
    """The forward rows of every selected cell: [(ms2 [S, n], pp7 [S, n], y0 [n], y1 [n])]."""
    n_sel, S, ld = theta.shape
    ms2, pp7 = lk.forward(theta.reshape(n_sel * S, ld), np.repeat(np.asarray(cid, np.int32), S), grid="interp")
    out = []
    for k, c in enumerate(cid):
        _, y0, y1 = lk.cells.cell(int(c))
        n = len(y0)
        out.append((ms2[k * S:(k + 1) * S, :n], pp7[k * S:(k + 1) * S, :n], y0, y1))
    return out


def tame_s2(rows, rng, S, zmax=30.0):
    """sigma2 [n_sel, S] with every |z| <= zmax: (largest finite |y - f| / zmax)^2 times U(1, 3)."""
    big = 1.0
    with np.errstate(invalid="ignore"):
        for m, p, y0, y1 in rows:
            for f, y in ((m, y0), (p, y1)):
                r = np.abs(y[None, :] - f)
                if np.any(np.isfinite(r)):
                    big = max(big, float(np.max(r[np.isfinite(r)])))
    return (big / zmax) ** 2 * rng.uniform(1.0, 3.0, (len(rows), S))


def check(lk, theta, s2, cid, levels=LEVELS, rows=None, **kw):
    """Likelihood.fitcheck against the restatement; returns the FitCheck."""
    rows = rows or sims(lk, theta, cid)
    got = lk.fitcheck(theta, s2, cid, levels=levels, **kw)
    n_sel, S, _ = theta.shape
    ld_out = int(lk.lengths[np.asarray(cid)].max())
    assert got.pit.shape == (n_sel, 2, ld_out) and got.coverage.shape == (n_sel, len(levels))
    worst = {"lppd_i": 0.0, "p_waic_i": 0.0, "pit": 0.0}
    for k, (m, p, y0, y1) in enumerate(rows):
        n = len(y0)
        ref = FO.cell(m, p, y0, y1, s2[k], levels)
        ex = FO.cell(m, p, y0, y1, s2[k], levels, exact=True)
        scored = ~np.isnan(ref["pit"])
        for f in FO.POINTWISE:
            g = getattr(got, f)[k]
            assert np.all(np.isnan(g[:, n:])), (k, f)
            want_nan = ~scored if not (S == 1 and f == "p_waic_i") else np.ones_like(scored)
            assert np.array_equal(np.isnan(g[:, :n]), want_nan), (k, f)
        for f in ("resid", "zbar", "z2"):
            assert np.array_equal(getattr(got, f)[k][:, :n], ref[f], equal_nan=True), (k, f)
        assert int(got.n_obs[k]) == ref["n_obs"] == int(scored.sum())
        b = FO.cell_bounds(ref, s2[k])
        for f in ("lppd_i", "p_waic_i", "pit"):
            if S == 1 and f == "p_waic_i":
                continue
            g = getattr(got, f)[k][:, :n][scored]
            bb, r64 = b[f][scored], ref[f][scored]
            e64 = np.abs(g - r64)
            eex = np.abs(np.float64(g.astype(np.longdouble) - ex[f][scored]))
            if g.size:
                worst[f] = max(worst[f], float(np.max(eex / bb)))
                print(f"cell {k} {f}: max |gpu - f64| / bound = {np.max(e64 / bb):.3g}, "
                      f"max |gpu - exact| / bound = {np.max(eex / bb):.3g}, max bound = {np.max(bb):.3g}")
            assert np.all(bb <= CAP * np.maximum(1.0, np.abs(r64))), (k, f)
            assert np.all(e64 <= 2.0 * bb), (k, f, float(np.max(e64 / bb)))
            assert np.all(eex <= bb), (k, f, float(np.max(eex / bb)))
        # the per-cell values are the host's sums over the pointwise vectors it returned
        mine = FO.per_cell({f: getattr(got, f)[k][:, :n] for f in FO.POINTWISE}, levels)
        assert mine["n_obs"] == int(got.n_obs[k])
        for f in ("lppd", "p_waic", "elpd_waic", "chi2"):
            assert np.array_equal(getattr(got, f)[k], mine[f], equal_nan=True), (k, f)
        assert np.array_equal(got.coverage[k], mine["coverage"], equal_nan=True)
        assert np.array_equal(got.dw[k], mine["dw"], equal_nan=True)
    return got


def fc_bytes(fc, k=None):
    fields = FO.POINTWISE + ("n_obs", "lppd", "p_waic", "elpd_waic", "chi2", "coverage", "dw")
    return b"".join((getattr(fc, f) if k is None else getattr(fc, f)[k]).tobytes() for f in fields)


@pytest.fixture(scope="module")
def lk(cells):
    from transcriptioncycleinference_amd import Likelihood

    with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as L:
        yield L


@pytest.fixture(scope="module")
def three(cells):
    """Three TestData cells of different N: the shortest, the median and the longest."""
    order = np.argsort(cells.lengths, kind="stable")
    cid = np.array([order[0], order[len(order) // 2], order[-1]], np.int32)
    assert len(set(cells.lengths[cid].tolist())) == 3
    return cid


def draw(rng, lengths, cid, S, ld=None):
    from test_predict_gpu import samples

    return samples(rng, lengths, cid, S, ld)


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 129, 500, 4096])
def test_sample_counts(lk, three, S):
    """The segment edges, one past an edge, the degenerate sizes and the cap."""
    rng = np.random.default_rng(200 + S)
    theta = draw(rng, lk.lengths, three, S)
    rows = sims(lk, theta, three)
    got = check(lk, theta, tame_s2(rows, rng, S), three, rows=rows)
    assert np.all(got.n_obs > 0) and np.all(np.isfinite(got.lppd)) and np.all(np.isfinite(got.chi2))
    assert np.all(np.isnan(got.p_waic)) if S == 1 else np.all(np.isfinite(got.elpd_waic))


def test_missing_data():
    """NaN data scattered in one dye, a dye that is all NaN, and a cell with no finite datum."""
    from transcriptioncycleinference_amd import Likelihood, from_lists
    from transcriptioncycleinference_amd.data import synthetic_times

    rng = np.random.default_rng(31)
    cl = []
    for n in (70, 131, 66):
        cl.append([synthetic_times(rng, n), rng.normal(3, 2, n), rng.normal(6, 3, n)])
    cl[0][1][rng.random(70) < 0.3] = np.nan
    cl[0][1][[0, 63, 64, 69]] = np.nan
    cl[1][2][:] = np.nan
    cl[2][1][:] = np.nan
    cl[2][2][:] = np.nan
    cid = np.array([2, 0, 1], np.int32)
    S = 70
    with Likelihood(from_lists([tuple(c) for c in cl]), "P2P-MS2v5-LacZ-PP7v4") as L:
        theta = draw(rng, L.lengths, cid, S)
        rows = sims(L, theta, cid)
        got = check(L, theta, tame_s2(rows, rng, S), cid, rows=rows)
    assert got.n_obs[0] == 0
    for f in ("lppd", "p_waic", "elpd_waic", "chi2"):
        assert np.isnan(getattr(got, f)[0]) and np.all(np.isfinite(getattr(got, f)[1:]))
    assert np.all(np.isnan(got.coverage[0])) and np.all(np.isnan(got.dw[0]))
    assert got.n_obs[1] == 70 + int(np.isfinite(cl[0][1]).sum()) and got.n_obs[2] == 131
    assert np.isnan(got.dw[2, 1]) and np.isfinite(got.dw[2, 0])     # the all-NaN dye: 0 / 0


def test_bad_sample_unscores_its_cell_only(lk, three):
    S = 66
    rng = np.random.default_rng(32)
    theta = draw(rng, lk.lengths, three, S)
    rows = sims(lk, theta, three)
    s2 = tame_s2(rows, rng, S)
    clean = lk.fitcheck(theta, s2, three, levels=LEVELS)
    theta[1, 65, 2] = np.nan
    got = check(lk, theta, s2, three)
    assert got.n_obs[1] == 0 and np.all(np.isnan(got.pit[1])) and np.isnan(got.elpd_waic[1])
    for k in (0, 2):
        assert fc_bytes(got, k) == fc_bytes(clean, k)


def test_out_of_posterior_sample(lk, three):
    """Data that the samples describe (the forward rows of one theta plus noise), and one sample far from them: its
    exp underflows to 0 and every output stays finite."""
    from transcriptioncycleinference_amd import Likelihood, from_lists

    S = 65
    rng = np.random.default_rng(33)
    cid = three[:2]
    base = draw(rng, lk.lengths, cid, 1)
    far = base.copy()
    far[:, :, 5] *= 1.5                                          # A: the whole MS2 signal half as large again
    fm, fp = lk.forward(base[:, 0], cid, grid="interp")
    gm, _ = lk.forward(far[:, 0], cid, grid="interp")
    sd0 = float(np.nanmax(np.abs(gm - fm))) / 300.0              # the far sample is at most 300 sd off: z^2 <= 10^5
    cl = []
    for k, c in enumerate(cid):
        t = lk.cells.cell(int(c))[0]
        n = len(t)
        cl.append((t, fm[k, :n] + rng.normal(0, sd0, n), fp[k, :n] + rng.normal(0, sd0, n)))
    sel = np.array([0, 1], np.int32)
    theta = np.repeat(base, S, axis=1)
    theta[:, :, 5] *= 1.0 + 0.0005 * rng.normal(size=(2, S))    # the near samples differ by a fraction of sd0
    theta[:, 40] = far[:, 0]
    s2 = sd0 ** 2 * rng.uniform(1.0, 1.5, (2, S))
    with Likelihood(from_lists(cl), "P2P-MS2v5-LacZ-PP7v4") as L:
        rows = sims(L, theta, sel)
        got = check(L, theta, s2, sel, rows=rows)
        for k, (m, _, y0, _) in enumerate(rows):
            ll = -0.5 * (np.log(FO.TWO_PI * s2[k])[:, None] + ((y0[None, :] - m) ** 2) / s2[k][:, None])
            under = np.exp(ll[40] - ll.max(axis=0)) == 0.0
            assert under.sum() >= 10                             # sample 40 underflows where the signal is large
            n = len(y0)
            for f in FO.POINTWISE:
                assert np.all(np.isfinite(getattr(got, f)[k][:, :n])), f
        assert np.all(np.isfinite(got.elpd_waic)) and np.all(got.n_obs == 2 * L.lengths[sel])


def test_short_cells_in_an_eight_rows_per_lane_context():
    """The cells of 2, 65 and 258 points of the rpl8 context of tests/ragged_cases.py: ld_out = 258, theta rows of 520
    entries, NaN past every cell's points."""
    import ragged_cases as RC
    from transcriptioncycleinference_amd import Likelihood, from_lists

    k = RC.case("rpl8", "builtin")
    lengths = [len(c[0]) for c in k.cl]
    cid = np.array([next(c for c in range(len(lengths)) if lengths[c] == n and not k.twin[c]) for n in (2, 258, 65)],
                   np.int32)
    S = 37
    rng = np.random.default_rng(258)
    with Likelihood(from_lists(k.cl), "P2P-MS2v5-LacZ-PP7v4") as L:
        assert L.info["rows_per_lane"] == 8 and L.lengths[cid].tolist() == [2, 258, 65]
        theta = draw(rng, L.lengths, cid, S, ld=k.ld)
        assert theta.shape == (3, S, 520)
        rows = sims(L, theta, cid)
        got = check(L, theta, tame_s2(rows, rng, S), cid, rows=rows)
    assert got.pit.shape == (3, 2, 258)
    for i, n in enumerate((2, 258, 65)):
        assert np.all(np.isnan(got.pit[i, :, n:])) and got.n_obs[i] > 0


def test_long_cell():
    """N = 600 runs the long-cell forward kernel; the tiles of 64 time points end ragged."""
    from test_parity_gpu import _long_cells
    from transcriptioncycleinference_amd import Likelihood

    rng = np.random.default_rng(600)
    cl = _long_cells(rng, 600)
    cid = np.array([0, 2, 1], np.int32)
    S = 9
    with Likelihood(cl, "P2P-MS2v5-LacZ-PP7v4") as L:
        assert L.info["rows_per_lane"] == 0 and int(L.lengths[cid].max()) == 600
        theta = draw(rng, L.lengths, cid, S)
        rows = sims(L, theta, cid)
        check(L, theta, tame_s2(rows, rng, S), cid, rows=rows)


def test_chunking_does_not_change_the_bytes(lk, three):
    from transcriptioncycleinference_amd import _lib

    S = 21
    rng = np.random.default_rng(34)
    cid = np.concatenate([three, three[::-1], three[:1]]).astype(np.int32)   # 7 selected cells
    theta = draw(rng, lk.lengths, cid, S)
    rows = sims(lk, theta, cid)
    s2 = tame_s2(rows, rng, S)
    whole = check(lk, theta, s2, cid, rows=rows)
    per_cell = 2 * S * int(lk.lengths[cid].max()) * 8
    for cap, chunks in ((2 * per_cell + 8, 4), (per_cell, 7)):
        assert -(-len(cid) // (cap // per_cell)) == chunks >= 3
        assert fc_bytes(lk.fitcheck(theta, s2, cid, levels=LEVELS, scratch_bytes=cap)) == fc_bytes(whole)
    with pytest.raises(_lib.TciError) as e:
        lk.fitcheck(theta, s2, cid, levels=LEVELS, scratch_bytes=per_cell - 1)
    assert e.value.code == _lib.TCI_EINVAL and "scratch" in str(e.value)
    assert fc_bytes(lk.fitcheck(theta, s2, cid, levels=LEVELS)) == fc_bytes(whole)   # the context still works


def test_layout_independence(lk, three):
    """The same cell at another position, with another n_sel, a longer ld_theta and (next to a longer cell) a longer
    ld_out: the same bytes."""
    S = 130
    rng = np.random.default_rng(35)
    theta = draw(rng, lk.lengths, three, S)
    s2 = tame_s2(sims(lk, theta, three), rng, S)
    a = lk.fitcheck(theta, s2, three, levels=LEVELS)
    alone = lk.fitcheck(theta[:1], s2[:1], three[:1], levels=LEVELS)
    wide = np.zeros((3, S, theta.shape[2] + 13))
    wide[:, :, :theta.shape[2]] = theta
    wide[:, :, theta.shape[2]:] = 7.5
    order = [2, 0, 1]
    b = lk.fitcheck(wide[order], s2[order], three[order], levels=LEVELS)
    n0 = int(lk.lengths[three[0]])
    assert alone.pit.shape[2] == n0 < a.pit.shape[2]
    for f in FO.POINTWISE:
        assert getattr(alone, f)[0][:, :n0].tobytes() == getattr(a, f)[0][:, :n0].tobytes(), f
    for f in ("n_obs", "lppd", "p_waic", "elpd_waic", "chi2", "coverage", "dw"):
        assert getattr(alone, f)[0].tobytes() == getattr(a, f)[0].tobytes(), f
    for i, k in enumerate(order):
        assert fc_bytes(b, i) == fc_bytes(a, k)


def test_tie_to_the_likelihood(lk, three):
    """S = 1: resid is y - f, and its squares over the scored points add up to the cell's SS."""
    from test_parity_gpu import REL

    rng = np.random.default_rng(36)
    theta = draw(rng, lk.lengths, three, 1)
    got = lk.fitcheck(theta, np.ones((3, 1)), three)
    ss = lk.ss_batch(theta[:, 0], three)
    for k in range(3):
        r = got.resid[k]
        mine = float(np.sum(r[~np.isnan(r)] ** 2))
        assert abs(mine - ss[k]) <= REL * abs(ss[k])
        assert np.array_equal(got.z2[k], got.resid[k] ** 2, equal_nan=True)   # sd = 1


def test_short_fit_then_fitcheck(lk, cells, tmp_path):
    import scipy.io as sio

    from transcriptioncycleinference_amd import mcmc

    ids = [0, 150, 298]
    fit = mcmc.fit(lk, n_steps=2000, n_burn=1000, seed=3, thin=5, cells=ids)
    rows = len(fit.MCMCchain[0]["v_chain"])
    assert rows == 200 and len(fit.MCMCchain[0]["s2chain"]) == 400
    assert mcmc.fitcheck(lk, fit, nsample=64, levels=LEVELS) is fit
    idx = mcmc.predict_rows(rows, 64)
    for k, c in enumerate(ids):
        n = int(cells.lengths[c])
        e = fit.MCMCcheck[k]
        th = mcmc.chain_theta(fit.MCMCchain[k], n, idx)[None]
        s2 = fit.MCMCchain[k]["s2chain"][-rows:][idx][None]
        cid = np.array([c], np.int32)
        one = check(lk, th, s2, cid)                       # the oracle on the selected rows
        for f in FO.POINTWISE:
            assert e[f].shape == (2, n) and np.array_equal(e[f], getattr(one, f)[0][:, :n], equal_nan=True)
        for f in ("lppd", "p_waic", "elpd_waic", "chi2"):
            assert e[f] == getattr(one, f)[0]
        assert e["n_obs"] == one.n_obs[0] and e["waic"] == -2.0 * e["elpd_waic"]
        assert np.array_equal(e["coverage"], one.coverage[0]) and np.array_equal(e["dw"], one.dw[0])
        assert e["levels"].tolist() == list(LEVELS) and e["n_samples"] == 64 and e["cell_index"] == c + 1
        assert 0.0 < e["chi2"] < 10.0 and np.all((e["coverage"] >= 0) & (e["coverage"] <= 1))
    res_path, _ = mcmc.save_results(fit, str(tmp_path), date="01-Jan-2021")
    d = sio.loadmat(res_path, squeeze_me=True, struct_as_record=False)
    for k, e in enumerate(np.atleast_1d(d["MCMCcheck"])):
        assert list(e._fieldnames) == list(mcmc.CHECK_FIELDS)
        for f in mcmc.CHECK_FIELDS:
            assert np.array_equal(np.asarray(getattr(e, f), np.float64),
                                  np.asarray(fit.MCMCcheck[k][f], np.float64), equal_nan=True), f
