"""Posterior covariance without a GPU: the longdouble restatement (tests/chaincov_oracle.py) against numpy on
well-conditioned data and against a one-pass FP64 formula on the near-constant column (where the one-pass
form fails), its NaN / padding rules, the MCMCcov schema and result-file round trip, and the argument checks
of the C ABI that come before any device call."""
import ctypes as C

import numpy as np
import pytest

import chaincov_oracle as O


def test_restatement_equals_numpy_on_well_conditioned_data():
    rng = np.random.default_rng(11)
    x = rng.standard_normal((400, 9)) @ rng.standard_normal((9, 9)) + rng.standard_normal(9)
    mean, cov, corr = O.moments(x)
    want_cov, want_corr = np.cov(x, rowvar=False, ddof=1), np.corrcoef(x, rowvar=False)
    assert np.max(np.abs(mean - x.mean(axis=0)) / np.abs(x.mean(axis=0))) <= 1e-13
    assert np.max(np.abs(cov - want_cov) / np.abs(want_cov)) <= 1e-13
    assert np.max(np.abs(corr - want_corr) / np.abs(want_corr)) <= 1e-13
    assert np.array_equal(cov, cov.T) and np.array_equal(corr, corr.T) and np.all(np.diagonal(corr) == 1.0)


def test_near_constant_column_needs_the_centred_form():
    """5 + 1e-6 noise: sum x^2 - n mean^2 in FP64 loses the variance, the two-pass form does not."""
    x = O.walk_chain(3, 1001, 1, 7)[:, 0, :]
    n = len(x)
    _, cov, _ = O.moments(x)
    v = x[:, 0]
    assert 1e-13 < cov[0, 0] < 1e-11
    one_pass = (np.sum(v * v) - n * np.mean(v) ** 2) / (n - 1)
    two_pass = np.sum((v - np.mean(v)) ** 2) / (n - 1)
    assert abs(two_pass - cov[0, 0]) / cov[0, 0] < 1e-9
    assert abs(one_pass - cov[0, 0]) / cov[0, 0] > 1e-6


def test_restatement_rules_for_special_columns_and_padding():
    x = O.walk_chain(5, 40, 2, 8, npar=[8, 5])
    x[:, 0, 3] = 0.1                      # a constant column
    x[7, 0, 4] = np.nan
    x[9, 0, 6] = np.inf
    t = O.table(x, [8, 5])
    m, cv, cr = t["mean"][0], t["cov"][0], t["corr"][0]
    assert m[3] == 0.1 and np.all(cv[3, [0, 1, 2, 3, 5, 7]] == 0.0) and np.all(np.isnan(cr[3])) and np.all(np.isnan(cr[:, 3]))
    for j in (4, 6):
        assert np.isnan(m[j]) and np.all(np.isnan(cv[j])) and np.all(np.isnan(cv[:, j])) and np.all(np.isnan(cr[:, j]))
    good = [0, 1, 2, 5, 7]
    assert np.all(np.isfinite(cv[np.ix_(good, good)])) and np.all(np.diagonal(cr)[good] == 1.0)
    assert np.all(np.abs(cr[np.ix_(good, good)]) <= 1.0) and cr[1, 2] < -0.99
    # padding of the second chain: NaN in all three, the real block finite
    assert np.all(np.isnan(t["mean"][1, 5:])) and np.all(np.isnan(t["cov"][1, 5:])) and np.all(np.isnan(t["corr"][1, :, 5:]))
    assert np.all(np.isfinite(t["cov"][1, :5, :5]))


def _fake_fit(with_cov):
    from transcriptioncycleinference_amd.mcmc import CHAIN_FIELDS, FitResult, PLOT_FIELDS, RESULT_FIELDS

    n = 5
    res = {f: (np.arange(n, dtype=float) if f.endswith("_dR") else 1.5) for f in RESULT_FIELDS}
    res["cell_index"], res["ApprovedFits"] = 3, 0
    plot = {f: np.arange(n, dtype=float) for f in PLOT_FIELDS}
    chain = {f: np.zeros((4, n) if f == "dR_chain" else 4) for f in CHAIN_FIELDS}
    cov = None
    if with_cov:
        P = 7 + n
        a = np.arange(float(P * P)).reshape(P, P)
        cov = [{"mean": np.arange(float(P)), "cov": a + a.T, "corr": np.eye(P), "n_rows": 301, "cell_index": 3}]
    return FitResult("unit", [res], [plot], [chain], np.array([0.3]), 10, 1.0, np.array([2]), MCMCcov=cov)


def test_cov_fields_and_result_file_round_trip(tmp_path):
    import scipy.io as sio

    from transcriptioncycleinference_amd.likelihood import ChainCov
    from transcriptioncycleinference_amd.mcmc import COV_FIELDS, DramResult, FitResult, cov_entry, save_results
    import dataclasses

    assert COV_FIELDS == ("mean", "cov", "corr", "n_rows", "cell_index")
    assert [f.name for f in dataclasses.fields(FitResult)][-1] == "MCMCcov"
    assert [f.name for f in dataclasses.fields(DramResult)][-1] == "cov"
    assert [f.name for f in dataclasses.fields(ChainCov)] == ["mean", "cov", "corr", "n_rows", "kernel_ms"]
    # cov_entry trims chain k to the cell's P = 7 + N
    cc = ChainCov.empty(2, 12)
    cc.n_rows = 301
    cc.mean[1, :10] = np.arange(10.0)
    cc.cov[1, :10, :10] = 2.0
    cc.corr[1, :10, :10] = 1.0
    e = cov_entry(cc, 1, 3, 42)
    assert tuple(e) == COV_FIELDS and e["n_rows"] == 301 and e["cell_index"] == 42
    assert e["mean"].tolist() == list(range(10)) and e["cov"].shape == (10, 10) == e["corr"].shape
    assert np.all(e["cov"] == 2.0) and np.all(e["corr"] == 1.0)
    # result files: MCMCcov only when the fit has it
    (tmp_path / "plain").mkdir()
    (tmp_path / "cov").mkdir()
    p0, _ = save_results(_fake_fit(False), str(tmp_path / "plain"), date="01-Jan-2024")
    p1, _ = save_results(_fake_fit(True), str(tmp_path / "cov"), date="01-Jan-2024")
    m0 = sio.loadmat(p0, squeeze_me=True, struct_as_record=False)
    m1 = sio.loadmat(p1, squeeze_me=True, struct_as_record=False)
    names = lambda m: {k for k in m if not k.startswith("__")}  # noqa: E731
    assert names(m0) == {"MCMCresults", "MCMCplot", "DatasetName"}          # the variables of every earlier fit
    assert names(m1) == names(m0) | {"MCMCcov"}
    cv = m1["MCMCcov"]
    want = _fake_fit(True).MCMCcov[0]
    assert tuple(cv._fieldnames) == COV_FIELDS and cv.n_rows == 301 and cv.cell_index == 3
    assert np.array_equal(cv.mean, want["mean"]) and np.array_equal(cv.cov, want["cov"]) and np.array_equal(cv.corr, want["corr"])
    assert tuple(m1["MCMCresults"]._fieldnames) == tuple(m0["MCMCresults"]._fieldnames)


def test_argument_checks_that_need_no_device():
    from transcriptioncycleinference_amd import _lib
    from transcriptioncycleinference_amd.build import build_library

    build_library()
    lib = _lib.load()
    o = _lib.tci_chaincov_options(77)
    assert lib.tci_chaincov_defaults(C.byref(o)) == _lib.TCI_OK and o.scratch_bytes == 0
    assert lib.tci_chaincov_defaults(None) == _lib.TCI_EINVAL
    out = _lib.tci_chaincov_outputs()
    x = np.zeros((20, 1, 1))
    assert lib.tci_chaincov(None, C.byref(o), _lib.ptr(x, _lib._dp), 20, 1, 1, None, C.byref(out)) == _lib.TCI_EINVAL
    dopt = _lib.tci_dram_options()
    dout = _lib.tci_dram_outputs()
    assert lib.tci_dram_run_cov(None, C.byref(dopt), 1, None, None, None, None, None, None, None, None, 8,
                                C.byref(dout), None, None, C.byref(o), C.byref(out)) == _lib.TCI_EINVAL
    # the Python wrapper's own checks come before the context is used
    from transcriptioncycleinference_amd.likelihood import Likelihood

    with pytest.raises(ValueError):
        Likelihood.chaincov(object(), np.zeros(5))
