"""Posterior predictive fit checks, the parts that need no GPU: the numpy restatement checked against closed forms and
against its own long-double path, every argument check of tci_fitcheck (they all come before any device work) and of
Likelihood.fitcheck, the row and sigma2 alignment of mcmc.fitcheck, and the result files with and without MCMCcheck."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
from scipy.special import erfc

import fitcheck_oracle as FO
from conftest import GOLDEN


@pytest.fixture(scope="module")
def lib():
    from transcriptioncycleinference_amd import _lib
    from transcriptioncycleinference_amd.build import build_library

    build_library()
    return _lib.load()


@pytest.fixture(scope="module")
def ctx(lib, cells):
    """A context over TestData cells 0..9; without a GPU its host-side cell table is still complete
    (tests/test_predict_host.py), which is all the argument checks read."""
    from transcriptioncycleinference_amd import _lib
    from transcriptioncycleinference_amd.construct import builtin_construct

    sub = cells.subset(range(10))
    cs, keep = builtin_construct("P2P-MS2v5-LacZ-PP7v4").to_c()
    tc = _lib.tci_cells(sub.n_cells, _lib.ptr(sub.offsets, _lib._i64p), _lib.ptr(sub.t, _lib._dp),
                        _lib.ptr(sub.ms2, _lib._dp), _lib.ptr(sub.pp7, _lib._dp))
    h = C.c_void_p()
    rc = lib.tci_create(C.byref(tc), C.byref(cs), 0, C.byref(h))
    assert rc in (_lib.TCI_OK, _lib.TCI_EHIP) and h.value
    yield h, sub
    lib.tci_destroy(h)


# ---- the restatement ----------------------------------------------------------------------------------------------


def test_equal_samples_closed_form():
    """All S samples equal: lppd = ll, p_waic = 0, pit = Phi(z), resid = r, zbar = z, z2 = z^2."""
    rng = np.random.default_rng(1)
    N, S = 7, 130
    f, y, s2 = rng.normal(5, 2, N), rng.normal(5, 2, N), 1.7
    sd, lg = math.sqrt(s2), math.log(FO.TWO_PI * s2)
    for exact in (False, True):
        o = FO.pointwise(np.repeat(f[None], S, 0), y, np.full(S, s2), exact=exact)
        z = (y - f) / sd
        ll = -0.5 * (lg + z * z)
        assert np.allclose(np.float64(o["lppd_i"]), ll, rtol=0, atol=1e-13)
        assert np.all(np.float64(o["p_waic_i"]) <= 1e-26)
        assert np.allclose(np.float64(o["pit"]), 0.5 * erfc(-z * FO.INV_SQRT2), rtol=0, atol=1e-14)
        assert np.allclose(np.float64(o["zbar"]), z, rtol=0, atol=1e-13)
    o = FO.pointwise(np.repeat(f[None], 64, 0), y, np.full(64, s2))  # one whole segment of equal terms
    assert np.allclose(o["resid"], y - f, rtol=0, atol=1e-14) and np.allclose(o["z2"], z * z, rtol=0, atol=1e-13)


def test_one_sample_has_no_penalty():
    o = FO.pointwise(np.array([[1.0, 2.0]]), np.array([1.5, 2.5]), np.array([0.3]))
    assert np.all(np.isnan(o["p_waic_i"])) and np.all(np.isfinite(o["lppd_i"])) and np.all(np.isfinite(o["pit"]))
    assert o["resid"].tolist() == [0.5, 0.5]


def test_unscored_points():
    """A NaN or infinite datum, and a point where any sample is not finite, are NaN in all six outputs."""
    sim = np.ones((3, 5))
    sim[1, 3] = np.nan
    sim[2, 4] = np.inf
    y = np.array([1.0, np.nan, np.inf, 1.0, 1.0])
    for exact in (False, True):
        o = FO.pointwise(sim, y, np.ones(3), exact=exact)
        for f in FO.POINTWISE:
            assert np.isnan(np.float64(o[f])).tolist() == [False, True, True, True, True], f
    c = FO.cell(sim, sim, y, np.full(5, np.nan), np.ones(3))
    assert c["n_obs"] == 1 and np.isnan(c["dw"][1]) and c["coverage"].tolist() == [1.0, 1.0]
    e = FO.cell(sim, sim, np.full(5, np.nan), np.full(5, np.nan), np.ones(3))
    assert e["n_obs"] == 0 and all(np.isnan(e[k]) for k in ("lppd", "p_waic", "elpd_waic", "chi2"))
    assert np.all(np.isnan(e["coverage"])) and np.all(np.isnan(e["dw"]))


def test_far_sample_contributes_exactly_zero():
    """A sample 800 nats below the maximum: exp underflows to 0, lppd is that of the others plus the log(S) shift, and
    nothing turns NaN."""
    y = np.array([0.0])
    near = np.zeros((4, 1))
    far = np.array([[40.0]])     # z = 40: ll = -800 - lg / 2
    s2 = np.ones(5)
    o = FO.pointwise(np.concatenate([near, far]), y, s2)
    o4 = FO.pointwise(near, y, s2[:4])
    assert math.exp(-800.0) == 0.0
    want = o4["lppd_i"][0] + math.log(4.0) - math.log(5.0)
    assert abs(o["lppd_i"][0] - want) <= 8 * FO.U * abs(want)
    assert all(np.isfinite(o[f][0]) for f in FO.POINTWISE)
    assert o["pit"][0] == (4 * 0.5 + 0.5 * erfc(40.0 * FO.INV_SQRT2)) / 5.0


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 129, 500, 4096])
def test_float64_path_is_within_the_bound_of_the_exact_path(S):
    rng = np.random.default_rng(50 + S)
    N = 12
    y = rng.normal(4, 3, N)
    sim = y[None, :] + rng.normal(0, 1, (S, N)) * rng.choice([0.5, 3.0, 40.0], N)[None, :]
    s2 = rng.uniform(0.2, 3.0, S)
    a, e = FO.pointwise(sim, y, s2), FO.pointwise(sim, y, s2, exact=True)
    _, lg, _ = FO.host_rows(s2)
    b = FO.bounds(S, a["Z2"], float(np.max(np.abs(lg))), a["lppd_i"], a["p_waic_i"])
    for f in ("lppd_i", "p_waic_i", "pit"):
        if S == 1 and f == "p_waic_i":
            assert np.all(np.isnan(a[f])) and np.all(np.isnan(np.float64(e[f])))
            continue
        err = np.abs(np.float64(a[f].astype(np.longdouble) - e[f]))
        assert np.all(err <= b[f]), (f, float(np.max(err / b[f])))
        assert np.all(b[f] <= 1e-10 * np.maximum(1.0, np.abs(a[f])))   # the bound itself stays a tight one
    for f in ("resid", "zbar", "z2"):
        err = np.abs(np.float64(a[f].astype(np.longdouble) - e[f]))
        assert np.all(err <= (min(S, 64) + S // 64 + 8) * FO.U * np.maximum(np.abs(a[f]), np.max(np.abs(sim - y))))


def test_segment_order():
    """seg_sum is the contract's order: not one running sum."""
    x = np.concatenate([[1.0], np.full(63, 2.0 ** -53), [1.0], np.full(63, 2.0 ** -53)])[:, None]
    part = 1.0
    for _ in range(63):
        part = part + 2.0 ** -53     # each addend is half an ulp of 1: ties to even, stays 1.0
    assert part == 1.0 and FO.seg_sum(x)[0] == 2.0
    assert FO.seg_sum(np.ones((130, 2))).tolist() == [130.0, 130.0]


def test_coverage_and_durbin_watson_by_hand():
    nan = np.nan
    pit = np.array([[0.1, 0.25, nan, 0.5, 0.75], [0.976, 0.024, 0.975, nan, nan]])
    zbar = np.array([[1.0, -1.0, nan, 2.0, 0.5], [0.5, 0.5, 1.5, nan, nan]])
    one = np.where(np.isnan(pit), nan, 1.0)
    pt = {"pit": pit, "zbar": zbar, "lppd_i": -2.0 * one, "p_waic_i": 0.25 * one, "z2": 3.0 * one}
    c = FO.per_cell(pt, (0.5, 0.95))
    assert c["n_obs"] == 7 and c["lppd"] == -14.0 and c["p_waic"] == 1.75 and c["elpd_waic"] == -15.75
    assert c["chi2"] == 3.0
    # level 0.5: [0.25, 0.75] holds 0.25, 0.5, 0.75; level 0.95: [0.025, 0.975] holds all but 0.976 and 0.024
    assert c["coverage"].tolist() == [3 / 7, 5 / 7]
    # dye 0: the pairs (0, 1) and (3, 4); the NaN at 2 breaks the run. dye 1: (0, 1) and (1, 2)
    assert c["dw"][0] == ((-2.0) ** 2 + (-1.5) ** 2) / (1 + 1 + 4 + 0.25)
    assert c["dw"][1] == (0.0 + 1.0) / (0.25 + 0.25 + 2.25)


# ---- the ABI's argument checks --------------------------------------------------------------------------------------


def test_defaults(lib):
    from transcriptioncycleinference_amd import _lib

    o = _lib.tci_fitcheck_options(7, 7, (C.c_double * 8)(*[9.0] * 8))
    assert lib.tci_fitcheck_defaults(C.byref(o)) == _lib.TCI_OK
    assert (o.scratch_bytes, o.n_levels, list(o.levels)) == (0, 2, [0.5, 0.95] + [0.0] * 6)
    assert lib.tci_fitcheck_defaults(None) == _lib.TCI_EINVAL


def test_abi_argument_checks(lib, ctx):
    from transcriptioncycleinference_amd import _lib

    h, sub = ctx
    n = int(sub.lengths.max())
    S, ld = 3, 7 + n
    theta = np.zeros((2, S, ld))
    s2 = np.ones((2, S))
    cid = np.array([0, 1], np.int32)
    outs = _lib.tci_fitcheck_outputs()
    P = lambda a, t=_lib._dp: _lib.ptr(a, t)  # noqa: E731

    def call(opt=None, theta=theta, ld=ld, s2=s2, cid=cid, n_sel=2, S=S, ld_out=n, h=h, out=outs):
        o = None
        if opt is not None:
            sb, lv = opt
            o = C.byref(_lib.tci_fitcheck_options(sb, len(lv), (C.c_double * 8)(*lv[:8])))
        rc = lib.tci_fitcheck(h, o, P(theta), ld, P(s2), P(cid, _lib._i32p), n_sel, S, ld_out,
                              None if out is None else C.byref(out))
        return rc, (lib.tci_last_error(h).decode() if h else "")

    assert call(h=None)[0] == _lib.TCI_EINVAL
    assert call(out=None)[0] == _lib.TCI_EINVAL
    for S_bad in (0, -1, 4097):
        rc, msg = call(S=S_bad)
        assert rc == _lib.TCI_EINVAL and "S=" in msg
    rc, msg = call(opt=(0, []))
    assert rc == _lib.TCI_EINVAL and "n_levels=0" in msg
    rc, msg = call(opt=(0, [0.5] * 9))
    assert rc == _lib.TCI_EINVAL and "n_levels=9" in msg
    for bad in (0.0, 1.0, -0.1, 1.5, np.nan, np.inf):
        rc, msg = call(opt=(0, [0.5, bad, 0.9]))
        assert rc == _lib.TCI_EINVAL and "levels[1]" in msg
    assert call(opt=(-1, [0.5]))[0] == _lib.TCI_EINVAL
    assert call(n_sel=-1)[0] == _lib.TCI_EINVAL
    for kw in (dict(theta=None), dict(s2=None), dict(cid=None)):
        assert call(**kw)[0] == _lib.TCI_EINVAL
    for bad in (0.0, -1.0, np.nan, np.inf):
        b = s2.copy()
        b[1, 2] = bad
        rc, msg = call(s2=b)
        assert rc == _lib.TCI_EINVAL and "s2[5]" in msg
    rc, msg = call(ld=7 + int(sub.lengths[:2].min()) - 1)
    assert rc == _lib.TCI_ERANGE and "theta needs" in msg                 # check_rows, as tci_predict
    rc, msg = call(cid=np.array([0, 10], np.int32))
    assert rc == _lib.TCI_ERANGE and "out of range" in msg
    rc, msg = call(ld_out=int(sub.lengths[:2].min()) - 1)
    assert rc == _lib.TCI_ERANGE and "ld_out" in msg
    rc, msg = call(opt=(2 * S * n * 8 - 1, [0.5]))                        # one cell alone does not fit
    assert rc == _lib.TCI_EINVAL and "scratch" in msg and str(2 * S * n * 8) in msg
    assert call(n_sel=0, theta=None, s2=None, cid=None)[0] == _lib.TCI_OK  # nothing selected: no device work


def test_binding_argument_checks(cells):
    from transcriptioncycleinference_amd import Likelihood

    lk = object.__new__(Likelihood)          # the checks run before the context is touched
    lk.lengths = cells.lengths.astype(np.int64)
    lk._h = None
    ld = 7 + int(cells.lengths.max())
    th, s2 = np.zeros((2, 3, ld)), np.ones((2, 3))
    bad_s2 = s2.copy()
    bad_s2[0, 1] = 0.0
    for kw in (dict(theta=th[0]), dict(cell_id=[0]), dict(cell_id=[0, 1, 2]), dict(s2=s2[0]), dict(s2=np.ones((2, 4))),
               dict(s2=bad_s2), dict(s2=np.full((2, 3), np.nan)), dict(levels=[]), dict(levels=[0.5] * 9),
               dict(levels=[0.5, 1.0]), dict(levels=[0.0]), dict(levels=[np.nan]), dict(levels=[[0.1, 0.2]]),
               dict(theta=np.zeros((2, 0, ld)), s2=np.ones((2, 0))),
               dict(theta=np.zeros((2, 4097, 9)), s2=np.ones((2, 4097))), dict(scratch_bytes=-1),
               dict(cell_id=[0, cells.n_cells]), dict(cell_id=[-1, 0])):
        args = dict(theta=th, s2=s2, cell_id=[0, 1])
        args.update(kw)
        with pytest.raises(ValueError):
            lk.fitcheck(**args)


# ---- mcmc.fitcheck and the result files ------------------------------------------------------------------------------


def _fake_fit(cells, rows, s2_rows=None):
    from transcriptioncycleinference_amd.mcmc import CHAIN_FIELDS, RESULT_FIELDS, FitResult

    rng = np.random.default_rng(1)
    res, plots, chains = [], [], []
    for c in (0, 1):
        t, m, p = cells.cell(c)
        n = len(t)
        r = {f: 0.5 for f in RESULT_FIELDS}
        r.update(mean_dR=np.zeros(n), sigma_dR=np.ones(n), cell_index=c + 1, ApprovedFits=0)
        res.append(r)
        plots.append({"t_plot": t, "MS2_plot": m, "PP7_plot": p, "simMS2": np.zeros(n), "simPP7": np.zeros(n)})
        ch = {f: rng.random(rows) for f in CHAIN_FIELDS}
        ch["dR_chain"] = rng.random((rows, n))
        ch["s2chain"] = 1.0 + rng.random(s2_rows or rows)   # unsliced by n_burn: longer than the chain rows
        chains.append(ch if rows else {})
    return FitResult("TestData", res, plots, chains, np.zeros(2), 0, 0.0, np.array([0, 1], np.int64))


class _FakeLk:
    """Records what mcmc.fitcheck hands to Likelihood.fitcheck and returns a recognisable FitCheck."""

    def __init__(self, cells):
        self.cells = cells
        self.calls = []

    def fitcheck(self, theta, s2, cell_id, levels=(0.5, 0.95), scratch_bytes=0):
        from transcriptioncycleinference_amd.likelihood import FITCHECK_POINTWISE, FitCheck

        self.calls.append((theta.copy(), s2.copy(), np.array(cell_id), tuple(levels), scratch_bytes))
        n_sel, S, _ = theta.shape
        fc = FitCheck.empty(n_sel, int(self.cells.lengths[np.asarray(cell_id)].max()), levels, S)
        for q, f in enumerate(FITCHECK_POINTWISE):
            getattr(fc, f)[:] = q + np.arange(n_sel)[:, None, None] * 10.0
        fc.n_obs[:] = 5
        fc.elpd_waic[:] = -3.0 - np.arange(n_sel)
        return fc


def test_mcmc_fitcheck_rows_and_sigma2_alignment(cells):
    """The theta rows are predict's; a row's sigma2 comes from the LAST len(v_chain) entries of s2chain."""
    from transcriptioncycleinference_amd import mcmc

    rows, s2_rows, nsample = 40, 100, 7
    fit = _fake_fit(cells, rows, s2_rows)
    lk = _FakeLk(cells)
    assert fit.MCMCcheck is None
    out = mcmc.fitcheck(lk, fit, nsample=nsample, levels=(0.8,), scratch_bytes=123)
    assert out is fit and len(lk.calls) == 1
    theta, s2, cid, levels, sb = lk.calls[0]
    idx = mcmc.predict_rows(rows, nsample)
    assert theta.shape == (2, nsample, 7 + int(cells.lengths[:2].max())) and cid.tolist() == [0, 1]
    assert levels == (0.8,) and sb == 123
    for k in (0, 1):
        n = int(cells.lengths[k])
        ch = fit.MCMCchain[k]
        assert np.array_equal(theta[k, :, :7 + n], mcmc.chain_theta(ch, n, idx))
        assert np.all(theta[k, :, 7 + n:] == 0)
        assert np.array_equal(s2[k], ch["s2chain"][s2_rows - rows:][idx])
        e = fit.MCMCcheck[k]
        assert list(e) == list(mcmc.CHECK_FIELDS)
        assert e["pit"].shape == (2, n) and np.all(e["pit"] == 2 + 10.0 * k) and np.all(e["z2"] == 5 + 10.0 * k)
        assert e["n_obs"] == 5 and e["elpd_waic"] == -3.0 - k and e["waic"] == 2 * (3.0 + k)
        assert e["levels"].tolist() == [0.8] and e["n_samples"] == nsample and e["cell_index"] == k + 1
    # column vectors, as save_results leaves the chains, select the same rows
    fit2 = _fake_fit(cells, rows, s2_rows)
    for ch in fit2.MCMCchain:
        for f in list(ch):
            if ch[f].ndim == 1:
                ch[f] = ch[f][:, None]
    lk2 = _FakeLk(cells)
    mcmc.fitcheck(lk2, fit2, nsample=nsample, levels=(0.8,))
    assert np.array_equal(lk2.calls[0][0], theta) and np.array_equal(lk2.calls[0][1], s2)
    with pytest.raises(ValueError, match="thin"):
        mcmc.fitcheck(lk, _fake_fit(cells, 0))
    with pytest.raises(ValueError, match="s2chain"):
        mcmc.fitcheck(lk, _fake_fit(cells, 10, 5))


def test_fit_result_keeps_positional_construction(cells):
    import dataclasses

    from transcriptioncycleinference_amd.mcmc import FitResult

    names = [f.name for f in dataclasses.fields(FitResult)]
    # among the optional fields that fit() sets by keyword (MCMCcov stays last), after every positional one
    assert names.index("rows_per_lane_uniform") + 1 == names.index("MCMCcheck") and names[-1] == "MCMCcov"
    assert _fake_fit(cells, 3).MCMCcheck is None


def test_result_files(cells, tmp_path):
    """A fit without MCMCcheck writes exactly the committed schema's variables; with it, one more, which loadmat
    gives back."""
    import scipy.io as sio

    from transcriptioncycleinference_amd import mcmc

    schema = json.load(open(os.path.join(GOLDEN, "result_schema.json")))["results_file"]
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    plain, _ = mcmc.save_results(_fake_fit(cells, 4), str(tmp_path / "a"), date="01-Jan-2021")
    d = sio.loadmat(plain, squeeze_me=True, struct_as_record=False)
    assert sorted(k for k in d if not k.startswith("__")) == sorted(schema["variables"])
    fit = mcmc.fitcheck(_FakeLk(cells), _fake_fit(cells, 4), nsample=3)
    fit.MCMCcheck[1]["pit"][0, 2] = np.nan
    with_check, _ = mcmc.save_results(fit, str(tmp_path / "b"), date="01-Jan-2021")
    d = sio.loadmat(with_check, squeeze_me=True, struct_as_record=False)
    assert sorted(k for k in d if not k.startswith("__")) == sorted(list(schema["variables"]) + ["MCMCcheck"])
    for k, e in enumerate(np.atleast_1d(d["MCMCcheck"])):
        assert list(e._fieldnames) == list(mcmc.CHECK_FIELDS)
        for f in mcmc.CHECK_FIELDS:
            assert np.array_equal(np.asarray(getattr(e, f), np.float64),
                                  np.asarray(fit.MCMCcheck[k][f], np.float64), equal_nan=True), f
