"""Posterior predictive envelopes on the device (tci_predict / k_quantile): the bands of
``Likelihood.predict`` against mcmcstat's plims rule, ``interp1(sort(x), (n-1)*p+1)``, written out in
numpy below and applied to the rows ``Likelihood.forward`` gives for the same theta. Sorting is exact
and the interpolation is one multiply and one add that are never fused, so the comparison is equality."""
import numpy as np
import pytest

from conftest import pack

pytestmark = pytest.mark.gpu

PROBS = (0.0, 0.025, 0.5, 0.975, 1.0)


def plims(sim, probs):
    """sim: [S, N] -> [nq, N]: x = sort over samples (NaN last); h = (S-1)*p; lo = floor(h); f = h - lo;
    x[lo] + f*(x[lo+1] - x[lo]) when lo + 1 < S, else x[S-1] (include/tci.h)."""
    x = np.sort(sim, axis=0)
    S = x.shape[0]
    out = np.empty((len(probs), x.shape[1]))
    with np.errstate(invalid="ignore"):
        for q, p in enumerate(probs):
            h = (S - 1) * p
            lo = int(np.floor(h))
            f = h - lo
            out[q] = x[lo] + f * (x[lo + 1] - x[lo]) if lo + 1 < S else x[S - 1]
    return out


def want_bands(lk, theta, cid, probs, grid):
    """The rule applied to lk.forward rows: [n_sel, nq, max N], NaN past a cell's N."""
    n_sel, S, ld = theta.shape
    ms2, pp7 = lk.forward(theta.reshape(n_sel * S, ld), np.repeat(np.asarray(cid, np.int32), S), grid=grid)
    ld_out = ms2.shape[1]
    wm, wp = np.full((n_sel, len(probs), ld_out), np.nan), np.full((n_sel, len(probs), ld_out), np.nan)
    for k in range(n_sel):
        n = int(lk.lengths[cid[k]])
        wm[k, :, :n] = plims(ms2[k * S:(k + 1) * S, :n], probs)
        wp[k, :, :n] = plims(pp7[k * S:(k + 1) * S, :n], probs)
    return wm, wp


def check(lk, theta, cid, probs=PROBS, grid="raw", **kw):
    gm, gp = lk.predict(theta, cid, probs=probs, grid=grid, **kw)
    wm, wp = want_bands(lk, theta, cid, probs, grid)
    assert gm.shape == wm.shape and gp.shape == wp.shape
    assert np.array_equal(gm, wm, equal_nan=True)
    assert np.array_equal(gp, wp, equal_nan=True)
    return gm, gp


def samples(rng, lengths, cid, S, ld=None):
    """S draws of the reference's x0 distribution per selected cell: [n_sel, S, ld]."""
    from transcriptioncycleinference_amd.data import draw_x0

    ld = ld or 7 + int(max(lengths[c] for c in cid))
    return np.stack([pack([draw_x0(rng, int(lengths[c])) for _ in range(S)], ld) for c in cid])


@pytest.fixture(scope="module")
def lk(cells):
    from transcriptioncycleinference_amd import Likelihood

    with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as L:
        yield L


@pytest.fixture(scope="module")
def three(cells):
    """Three TestData cells of different N (time tiles end ragged)."""
    order = np.argsort(cells.lengths, kind="stable")
    cid = np.array([order[0], order[len(order) // 2], order[-1]], np.int32)
    assert len(set(cells.lengths[cid].tolist())) == 3
    return cid


@pytest.mark.parametrize("S", [1, 2, 3, 5, 37, 64, 65, 500, 4096])
def test_sample_counts(lk, three, S):
    """Powers of two, one past a power of two, the degenerate sizes and the cap; p = 0, p = 1 and h on
    an integer (S = 5, p = 0.5)."""
    theta = samples(np.random.default_rng(100 + S), lk.lengths, three, S)
    gm, gp = check(lk, theta, three)
    for k, c in enumerate(three):
        n = int(lk.lengths[c])
        assert not np.any(np.isnan(gm[k, :, :n])) and np.all(np.isnan(gm[k, :, n:]))
        assert not np.any(np.isnan(gp[k, :, :n])) and np.all(np.isnan(gp[k, :, n:]))


def test_duplicated_samples(lk, three):
    """All S rows equal: every band is the forward row."""
    one = samples(np.random.default_rng(7), lk.lengths, three, 1)
    theta = np.repeat(one, 33, axis=1)
    gm, gp = check(lk, theta, three)
    fm, fp = lk.forward(one[:, 0], three, grid="raw")
    for q in range(len(PROBS)):
        assert np.array_equal(gm[:, q], fm, equal_nan=True) and np.array_equal(gp[:, q], fp, equal_nan=True)


def test_nan_sample_sorts_last(lk, three):
    """A NaN entry in one theta row makes that sample all NaN: it sorts last, so the bands whose
    bracket reaches the last sample are NaN and the lower ones are not."""
    S = 41
    theta = samples(np.random.default_rng(8), lk.lengths, three, S)
    theta[0, 17, 2] = np.nan
    theta[2, 0, 9] = np.nan
    gm, gp = check(lk, theta, three)   # x[40] is the NaN sample: p = 1 reads it, p = 0 and the median do not
    n = [int(lk.lengths[c]) for c in three]
    for k in (0, 2):
        for g in (gm, gp):
            assert np.all(np.isfinite(g[k, [0, 2], :n[k]])) and np.all(np.isnan(g[k, 4, :n[k]]))
    assert np.all(np.isfinite(gm[1, :, :n[1]])) and np.all(np.isfinite(gp[1, :, :n[1]]))


def test_interp_grid(lk, three):
    """grid='interp': through the uniform grid + interp1 as inside the SS; where a cell's grid does
    not cover a time the simulated value, hence every band there, is NaN (the numpy rule carries the
    NaN through). No TestData cell and none of 16,000 random synthetic cells has such a time: the
    colon rule snaps the grid's last point to t(end), so the case runs on cells whose grid covers all."""
    theta = samples(np.random.default_rng(9), lk.lengths, three, 29)
    gm, _ = check(lk, theta, three, grid="interp")
    rm, _ = lk.predict(theta, three, probs=PROBS, grid="raw")
    assert not np.array_equal(gm, rm, equal_nan=True)   # the two grids are different models


def test_long_cell(construct):
    """N = 600 runs the long-cell forward kernel; time tiles of 64 end ragged at 600, 593, 586."""
    from transcriptioncycleinference_amd import Likelihood
    from test_parity_gpu import _long_cells

    rng = np.random.default_rng(600)
    cl = _long_cells(rng, 600)
    cid = np.array([0, 2, 1], np.int32)
    with Likelihood(cl, "P2P-MS2v5-LacZ-PP7v4") as L:
        assert L.info["rows_per_lane"] == 0
        check(L, samples(rng, L.lengths, cid, 8), cid)


def test_short_cells_in_an_eight_rows_per_lane_context():
    """The cells of 2, 65 and 258 points of a context whose longest cell has 513 (tests/ragged_cases.py,
    RPL = 8) in one call, S = 37, both grids: the forward kernel on padded records, ld_out = 258 with 256
    and 193 NaN entries past the short cells' points, theta rows of 520 entries."""
    import ragged_cases as RC
    from transcriptioncycleinference_amd import Likelihood, from_lists

    k = RC.case("rpl8", "builtin")
    lengths = [len(c[0]) for c in k.cl]
    cid = np.array([next(c for c in range(len(lengths)) if lengths[c] == n and not k.twin[c]) for n in (2, 258, 65)],
                   np.int32)
    with Likelihood(from_lists(k.cl), "P2P-MS2v5-LacZ-PP7v4") as L:
        assert L.info["rows_per_lane"] == 8 and L.lengths[cid].tolist() == [2, 258, 65]
        theta = samples(np.random.default_rng(258), L.lengths, cid, 37, ld=k.ld)
        assert theta.shape == (3, 37, 520)
        for grid in ("raw", "interp"):
            gm, gp = check(L, theta, cid, grid=grid)
            assert gm.shape == gp.shape == (3, len(PROBS), 258)
            for i, n in enumerate((2, 258, 65)):
                assert np.all(np.isnan(gm[i, :, n:])) and np.all(np.isnan(gp[i, :, n:]))
                if grid == "raw":  # the raw grid covers every acquisition time
                    assert np.all(np.isfinite(gm[i, :, :n])) and np.all(np.isfinite(gp[i, :, :n]))


def test_four_segment_construct():
    from transcriptioncycleinference_amd import Likelihood, from_lists
    from transcriptioncycleinference_amd.construct import Construct
    from transcriptioncycleinference_amd.data import synthetic_times

    a = np.linspace(0.05, 9.0, 4)
    cs = Construct(11.0, list(a), list(a + 0.8), [24.0, 12.0, 6.0, 24.0], list(a + 0.3), list(a + 1.9), [24.0] * 4,
                   "seg4")
    rng = np.random.default_rng(4)
    cl = from_lists([(synthetic_times(rng, n), rng.normal(3, 2, n), rng.normal(6, 3, n)) for n in (70, 131)])
    cid = np.array([1, 0], np.int32)
    with Likelihood(cl, cs) as L:
        check(L, samples(rng, L.lengths, cid, 19), cid)


def test_chunking_does_not_change_the_bands(lk, three):
    from transcriptioncycleinference_amd import _lib

    S = 21
    cid = np.concatenate([three, three[::-1], three[:1]]).astype(np.int32)   # 7 selected cells
    theta = samples(np.random.default_rng(10), lk.lengths, cid, S)
    whole = lk.predict(theta, cid, probs=PROBS)
    per_cell = 2 * S * int(lk.lengths[cid].max()) * 8
    for cap, chunks in ((2 * per_cell + 8, 4), (per_cell, 7)):
        assert -(-len(cid) // (cap // per_cell)) == chunks >= 3
        got = lk.predict(theta, cid, probs=PROBS, scratch_bytes=cap)
        for g, w in zip(got, whole):
            assert g.tobytes() == w.tobytes()
    with pytest.raises(_lib.TciError) as e:
        lk.predict(theta, cid, probs=PROBS, scratch_bytes=per_cell - 1)
    assert e.value.code == _lib.TCI_EINVAL and "scratch" in str(e.value)
    check(lk, theta, cid)   # the context still works after the refusal


def test_permutation_invariance(lk, three):
    S = 100
    rng = np.random.default_rng(11)
    theta = samples(rng, lk.lengths, three, S)
    gm, gp = lk.predict(theta, three, probs=PROBS)
    perm = np.stack([theta[k, rng.permutation(S)] for k in range(len(three))])
    pm, pq = lk.predict(perm, three, probs=PROBS)
    assert np.array_equal(gm, pm, equal_nan=True) and np.array_equal(gp, pq, equal_nan=True)


def test_bands_vs_oracle_forward(lk, three, cells, construct, c_oracle):
    """The same rule on the CPU oracle's forward rows, at the project's forward-parity tolerance."""
    from test_parity_gpu import REL, rel_err

    S = 12
    theta = samples(np.random.default_rng(12), lk.lengths, three, S)
    gm, gp = lk.predict(theta, three, probs=PROBS)
    for k, c in enumerate(three):
        t = cells.cell(int(c))[0]
        rows = [c_oracle.forward(t, construct, theta[k, s, :7 + len(t)], mode=0) for s in range(S)]
        wm, wp = plims(np.stack([r[0] for r in rows]), PROBS), plims(np.stack([r[1] for r in rows]), PROBS)
        assert rel_err(gm[k, :, :len(t)], wm) <= REL and rel_err(gp[k, :, :len(t)], wp) <= REL


def test_abi_range_errors_and_empty_call(lk, three):
    from transcriptioncycleinference_amd import _lib

    theta = samples(np.random.default_rng(13), lk.lengths, three, 4)
    with pytest.raises(_lib.TciError) as e:
        lk.predict(theta[:, :, :60], three)           # ld_theta < 7 + N
    assert e.value.code == _lib.TCI_ERANGE
    gm, gp = lk.predict(theta[:0], three[:0])         # n_sel == 0
    assert gm.shape == (0, 3, 1) and gp.shape == (0, 3, 1)


def test_short_fit_then_predict(lk, cells, tmp_path):
    import scipy.io as sio

    from transcriptioncycleinference_amd import mcmc

    ids = [0, 150, 298]
    fit = mcmc.fit(lk, n_steps=2000, n_burn=1000, seed=3, thin=5, cells=ids)
    rows = len(fit.MCMCchain[0]["v_chain"])
    assert rows == 200
    mcmc.predict(lk, fit, nsample=64)
    for k, c in enumerate(ids):
        n = int(cells.lengths[c])
        p = fit.MCMCplot[k]
        assert p["predMS2"].shape == (3, n) and p["predPP7"].shape == (3, n)
        assert np.array_equal(p["pred_probs"], [0.025, 0.5, 0.975])
        assert np.all(np.isfinite(p["predMS2"][1][np.isfinite(p["simMS2"])]))
        assert np.all(np.isfinite(p["predPP7"][1][np.isfinite(p["simPP7"])]))
        # the bands are the rule on the forward rows of the selected chain rows
        th = mcmc.chain_theta(fit.MCMCchain[k], n, mcmc.predict_rows(rows, 64))
        wm, wp = want_bands(lk, th[None], np.array([c], np.int32), (0.025, 0.5, 0.975), "raw")
        assert np.array_equal(p["predMS2"], wm[0, :, :n]) and np.array_equal(p["predPP7"], wp[0, :, :n])
    res_path, _ = mcmc.save_results(fit, str(tmp_path), date="01-Jan-2021")
    d = sio.loadmat(res_path, squeeze_me=True, struct_as_record=False)
    for k, p in enumerate(np.atleast_1d(d["MCMCplot"])):
        assert np.array_equal(p.predMS2, fit.MCMCplot[k]["predMS2"])
        assert np.array_equal(p.predPP7, fit.MCMCplot[k]["predPP7"])
        assert np.array_equal(p.pred_probs, [0.025, 0.5, 0.975])
