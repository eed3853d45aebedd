"""Predictive envelopes, the parts that need no GPU: every argument check of tci_predict (they all come
before any device work), of Likelihood.predict and of tci_mex('predict'), the row-selection rule
of mcmc.predict, and the result files of a fit without predict."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def lib():
    from transcriptioncycleinference_amd import _lib
    from transcriptioncycleinference_amd.build import build_library

    build_library()
    return _lib.load()


@pytest.fixture(scope="module")
def ctx(lib, cells):
    """A context over TestData cells 0..9. Without a GPU tci_create fails at its first HIP call and
    still hands the context back (for tci_last_error): its host-side cell table is complete, which is
    all the argument checks of tci_predict read."""
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


def test_defaults(lib):
    from transcriptioncycleinference_amd import _lib

    o = _lib.tci_predict_options(7, 7)
    assert lib.tci_predict_defaults(C.byref(o)) == _lib.TCI_OK
    assert (o.grid_mode, o.scratch_bytes) == (_lib.TCI_GRID_RAW, 0)
    assert lib.tci_predict_defaults(None) == _lib.TCI_EINVAL


def test_abi_argument_checks(lib, ctx):
    from transcriptioncycleinference_amd import _lib

    h, sub = ctx
    n = int(sub.lengths.max())
    S, ld = 3, 7 + n
    theta = np.zeros((2, S, ld))
    cid = np.array([0, 1], np.int32)
    probs = np.array([0.025, 0.5, 0.975])
    out = np.zeros((2, 2, 3, n))
    P = lambda a, t=_lib._dp: _lib.ptr(a, t)  # noqa: E731

    def call(opt=None, theta=theta, ld=ld, cid=cid, n_sel=2, S=S, probs=probs, nq=3, ld_out=n, h=h, ms2=out[0]):
        o = None if opt is None else C.byref(_lib.tci_predict_options(*opt))
        rc = lib.tci_predict(h, o, P(theta), ld, P(cid, _lib._i32p), n_sel, S, P(probs), nq, P(ms2), P(out[1]), ld_out)
        return rc, (lib.tci_last_error(h).decode() if h else "")

    assert call(h=None)[0] == _lib.TCI_EINVAL
    for S_bad in (0, -1, 4097):
        rc, msg = call(S=S_bad)
        assert rc == _lib.TCI_EINVAL and "S=" in msg
    for nq_bad in (0, 17):
        rc, msg = call(nq=nq_bad, probs=np.full(17, 0.5))
        assert rc == _lib.TCI_EINVAL and "nq=" in msg
    for bad in (-0.1, 1.0000001, np.nan, np.inf):
        rc, msg = call(probs=np.array([0.5, bad, 0.5]))
        assert rc == _lib.TCI_EINVAL and "probs[1]" in msg
    assert call(probs=None)[0] == _lib.TCI_EINVAL
    rc, msg = call(opt=(2, 0))
    assert rc == _lib.TCI_EINVAL and "grid_mode" in msg
    assert call(opt=(_lib.TCI_GRID_RAW, -1))[0] == _lib.TCI_EINVAL
    assert call(n_sel=-1)[0] == _lib.TCI_EINVAL
    assert call(theta=None)[0] == _lib.TCI_EINVAL and call(cid=None)[0] == _lib.TCI_EINVAL
    assert call(ms2=None)[0] == _lib.TCI_EINVAL
    rc, msg = call(ld=7 + int(sub.lengths[:2].min()) - 1)
    assert rc == _lib.TCI_ERANGE and "theta needs" in msg                 # as tci_forward: check_rows
    rc, msg = call(cid=np.array([0, 10], np.int32))
    assert rc == _lib.TCI_ERANGE and "out of range" in msg
    rc, msg = call(ld_out=int(sub.lengths[:2].min()) - 1)
    assert rc == _lib.TCI_ERANGE and "ld_out" in msg
    rc, msg = call(opt=(_lib.TCI_GRID_RAW, 2 * S * n * 8 - 1))            # one cell alone does not fit
    assert rc == _lib.TCI_EINVAL and "scratch" in msg and str(2 * S * n * 8) in msg
    assert call(n_sel=0, theta=None, cid=None)[0] == _lib.TCI_OK          # nothing selected: no device work


def test_binding_argument_checks(cells):
    from transcriptioncycleinference_amd import Likelihood

    lk = object.__new__(Likelihood)          # the checks run before the context is touched
    lk.lengths = cells.lengths.astype(np.int64)
    lk._h = None
    ld = 7 + int(cells.lengths.max())
    th = np.zeros((2, 3, ld))
    for kw in (dict(theta=th[0]), dict(cell_id=[0]), dict(cell_id=[0, 1, 2]), dict(probs=[]), dict(probs=[0.5] * 17),
               dict(probs=[0.5, 1.5]), dict(probs=[np.nan]), dict(probs=[[0.1, 0.2]]), dict(grid="uniform"),
               dict(theta=np.zeros((2, 0, ld))), dict(theta=np.zeros((2, 4097, 9))), dict(scratch_bytes=-1),
               dict(cell_id=[0, cells.n_cells]), dict(cell_id=[-1, 0])):
        args = dict(theta=th, cell_id=[0, 1])
        args.update(kw)
        with pytest.raises(ValueError):
            lk.predict(**args)


def test_row_selection_rule():
    from transcriptioncycleinference_amd.mcmc import predict_rows

    assert np.array_equal(predict_rows(7, 500), np.arange(7))             # fewer rows than nsample: all of them
    assert np.array_equal(predict_rows(500, 500), np.arange(500))
    assert np.array_equal(predict_rows(10, 4), np.round(np.linspace(0, 9, 4)).astype(int))
    idx = predict_rows(10001, 500)
    assert len(idx) == 500 and idx[0] == 0 and idx[-1] == 10000 and np.all(np.diff(idx) > 0)
    assert np.array_equal(idx, np.round(np.linspace(0, 10000, 500)))
    assert np.array_equal(predict_rows(3, 1), [0])
    with pytest.raises(ValueError):
        predict_rows(10, 0)


def _fake_fit(cells, rows, pred=False):
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
        if pred:
            plots[-1].update(predMS2=rng.random((3, n)), predPP7=rng.random((3, n)),
                             pred_probs=np.array([0.025, 0.5, 0.975]))
        ch = {f: rng.random(rows) for f in CHAIN_FIELDS}
        ch["dR_chain"] = rng.random((rows, n))
        chains.append(ch if rows else {})
    return FitResult("TestData", res, plots, chains, np.zeros(2), 0, 0.0, np.array([0, 1], np.int64))


def test_chain_theta_is_in_abi_order(cells):
    from transcriptioncycleinference_amd.mcmc import chain_theta

    fit = _fake_fit(cells, 6)
    ch, n = fit.MCMCchain[1], int(cells.lengths[1])
    idx = np.array([0, 2, 5])
    th = chain_theta(ch, n, idx)
    assert th.shape == (3, 7 + n)
    for col, name in enumerate(("v", "tau", "ton", "MS2_basal", "PP7_basal", "A", "R")):   # include/tci.h
        assert np.array_equal(th[:, col], ch[name + "_chain"][idx])
    assert np.array_equal(th[:, 7:], ch["dR_chain"][idx])
    # column vectors, as save_results leaves the chains
    col = {k: (v[:, None] if v.ndim == 1 else v) for k, v in ch.items()}
    assert np.array_equal(chain_theta(col, n, idx), th)


def test_predict_without_chain_rows_raises(cells):
    from transcriptioncycleinference_amd import mcmc

    with pytest.raises(ValueError, match="thin"):
        mcmc.predict(None, _fake_fit(cells, 0))


def test_result_files_without_predict_are_unchanged(cells, tmp_path):
    """A fit without predict writes exactly the committed schema's fields; with the bands, three more."""
    import scipy.io as sio

    from transcriptioncycleinference_amd import mcmc

    schema = json.load(open(os.path.join(GOLDEN, "result_schema.json")))["results_file"]
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    plain, _ = mcmc.save_results(_fake_fit(cells, 4), str(tmp_path / "a"), date="01-Jan-2021")
    d = sio.loadmat(plain, squeeze_me=True, struct_as_record=False)
    assert sorted(k for k in d if not k.startswith("__")) == sorted(schema["variables"])
    assert list(d["MCMCplot"][0]._fieldnames) == list(schema["MCMCplot"]) == list(mcmc.PLOT_FIELDS)
    assert list(d["MCMCresults"][0]._fieldnames) == list(schema["MCMCresults"])
    with_pred, _ = mcmc.save_results(_fake_fit(cells, 4, pred=True), str(tmp_path / "b"), date="01-Jan-2021")
    d = sio.loadmat(with_pred, squeeze_me=True, struct_as_record=False)
    assert list(d["MCMCplot"][0]._fieldnames) == list(mcmc.PLOT_FIELDS + mcmc.PRED_FIELDS)
    assert d["MCMCplot"][1].predMS2.shape == (3, int(cells.lengths[1]))
