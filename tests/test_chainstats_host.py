"""Chain diagnostics without a GPU: the numpy oracle (tests/chainstats_oracle.py) against hand-computed
values, its FFT form against the direct lag form, the MCMCdiag schema and result-file round trip, and
the argument checks of the C ABI that come before any device call."""
import ctypes as C
import math

import numpy as np
import pytest

import chainstats_oracle as O


def test_oracle_equals_hand_computed_values_on_20_rows():
    # the ramp 1 .. 20: b = 10, two batches with means 5.5 and 15.5 around 10.5:
    # s = sqrt(10 * (25 + 25) / 1) = sqrt(500), mcerr = sqrt(500 / 20) = 5
    x = np.arange(1.0, 21.0)
    assert O.bm_s(x) == pytest.approx(math.sqrt(500.0), rel=1e-15)
    assert O.mcerr(x) == pytest.approx(5.0, rel=1e-15)
    assert math.isnan(O.mcerr(x[:19]))
    # y = -9.5 .. 9.5: c(0) = 665; c(1) = (665 - 90.25) - 9.5 + 9.5 * (-9.5) = 475
    c = O.acov_direct(x)
    assert c[0] == pytest.approx(665.0, rel=1e-15) and c[1] == pytest.approx(475.0, rel=1e-15)
    # the alternating column +1, -1: rho(k) = (-1)^k. S = -1/3 -> 1/2 (i = 1) -> -2/3 (i = 2): the
    # window closes at i = 2 with tau = 2 (-2/3 + 1/6) = -1; its batches of 10 all average 0
    a = np.tile([1.0, -1.0], 10)
    tau, w, margin = O.sokal(O.acov_fft(a))
    assert (w, tau) == (2, pytest.approx(-1.0, abs=1e-15)) and margin == pytest.approx(0.5)
    assert O.mcerr(a) == 0.0
    # max_lag = 1: no crossing within one lag
    assert O.sokal(O.acov_fft(a), 1) == (math.inf, 1, pytest.approx(0.5))
    # Geweke needs 20 rows in the first tenth; a constant column is 0/0; one NaN spoils the column
    assert all(math.isnan(v) for v in O.geweke(np.arange(199.0)))
    r = O.column(np.full(257, 3.0))
    assert (r["tau"], r["tau_window"], r["mcerr"]) == (0.0, 0, 0.0) and math.isnan(r["geweke_z"]) and math.isnan(r["geweke_p"])
    bad = np.arange(300.0)
    bad[17] = np.nan
    r = O.column(bad)
    assert r["tau_window"] == -1 and all(math.isnan(r[k]) for k in ("mcerr", "tau", "geweke_z", "geweke_p"))
    # two segments with equal batch means but shifted levels: z from the formula by hand
    g = np.concatenate([np.tile([0.0, 2.0], 50), np.tile([4.0, 6.0], 150)])   # n = 400: A = 40 rows, B = 200
    # A: b = 10, every batch mean = 1 = mean_A -> s_A = 0; B likewise -> z = -4 / 0 = -Inf, p = 0
    z, p = O.geweke(g)
    assert z == -math.inf and p == 0.0


def test_fft_form_equals_the_direct_lag_form():
    x = O.ar1_columns(np.random.default_rng(7), 257, 200)
    worst, windows, margin = 0.0, set(), math.inf
    for j in range(x.shape[1]):
        f, d = O.column(x[:, j]), O.column(x[:, j], direct=True)
        assert f["tau_window"] == d["tau_window"]
        worst = max(worst, abs(f["tau"] - d["tau"]) / abs(d["tau"]))
        windows.add(f["tau_window"])
        margin = min(margin, f["margin"], d["margin"])
    assert worst < 1e-13
    assert margin >= 1e-6            # no column's running sum comes near zero before it crosses
    assert min(windows) < 8 and max(windows) > 64   # the windows span more than one 64-lag tile


def _fake_fit(with_diag):
    from transcriptioncycleinference_amd.mcmc import CHAIN_FIELDS, DIAG_FIELDS, FitResult, PLOT_FIELDS, RESULT_FIELDS

    n = 5
    res = {f: (np.arange(n, dtype=float) if f.endswith("_dR") else 1.5) for f in RESULT_FIELDS}
    res["cell_index"], res["ApprovedFits"] = 3, 0
    plot = {f: np.arange(n, dtype=float) for f in PLOT_FIELDS}
    chain = {f: np.zeros((4, n) if f == "dR_chain" else 4) for f in CHAIN_FIELDS}
    diag = None
    if with_diag:
        d = {f: (np.arange(n, dtype=float) + 0.25 if f.endswith("_dR") else 2.5) for f in DIAG_FIELDS}
        d["n_rows"], d["cell_index"], d["ess_min"] = 1501, 3, 12.5
        diag = [d]
    return FitResult("unit", [res], [plot], [chain], np.array([0.3]), 10, 1.0, np.array([2]), MCMCdiag=diag)


def test_diag_fields_and_result_file_round_trip(tmp_path):
    import scipy.io as sio

    from transcriptioncycleinference_amd.likelihood import ChainStats
    from transcriptioncycleinference_amd.mcmc import DIAG_FIELDS, diag_entry, save_results

    names = ("v", "ton", "A", "tau", "MS2_basal", "PP7_basal", "R", "dR", "s2")
    assert DIAG_FIELDS == tuple(f"{s}_{n}" for s in ("mcerr", "tau", "geweke_p") for n in names) + (
        "n_rows", "ess_min", "cell_index")
    # diag_entry: theta order [v, tau, ton, MS2_basal, PP7_basal, A, R, dR..]; ess_min = n_rows / max tau
    st = ChainStats.empty(2, 12)
    st.n_rows = 1000
    st.tau[1, :10] = [4.0, 1.0, 2.0, 3.0, 5.0, 6.0, 7.0, 8.0, 50.0, 9.0]
    st.tau[1, 10:] = np.nan                      # padding of a 3-point cell
    st.s2_tau[1] = 400.0                         # s2 does not enter ess_min
    d = diag_entry(st, 1, 3, 42)
    assert tuple(d) == DIAG_FIELDS
    assert (d["tau_v"], d["tau_tau"], d["tau_ton"], d["tau_A"], d["tau_R"]) == (4.0, 1.0, 2.0, 6.0, 7.0)
    assert d["tau_dR"].tolist() == [8.0, 50.0, 9.0] and d["tau_s2"] == 400.0
    assert d["ess_min"] == 20.0 and d["n_rows"] == 1000 and d["cell_index"] == 42
    st.tau[1, 2] = np.inf
    assert diag_entry(st, 1, 3, 42)["ess_min"] == 0.0
    # result files: MCMCdiag only when the fit has it
    (tmp_path / "plain").mkdir()
    (tmp_path / "diag").mkdir()
    p0, _ = save_results(_fake_fit(False), str(tmp_path / "plain"), date="01-Jan-2024")
    p1, _ = save_results(_fake_fit(True), str(tmp_path / "diag"), date="01-Jan-2024")
    m0 = sio.loadmat(p0, squeeze_me=True, struct_as_record=False)
    m1 = sio.loadmat(p1, squeeze_me=True, struct_as_record=False)
    assert "MCMCdiag" not in m0 and {"MCMCresults", "MCMCplot", "DatasetName"} <= set(m0)
    dg = m1["MCMCdiag"]
    assert tuple(dg._fieldnames) == DIAG_FIELDS
    assert dg.n_rows == 1501 and dg.cell_index == 3 and dg.ess_min == 12.5 and dg.tau_s2 == 2.5
    assert np.array_equal(dg.mcerr_dR, np.arange(5.0) + 0.25)
    assert tuple(m1["MCMCresults"]._fieldnames) == tuple(m0["MCMCresults"]._fieldnames)


def test_argument_checks_that_need_no_device():
    from transcriptioncycleinference_amd import _lib
    from transcriptioncycleinference_amd.build import build_library

    build_library()
    lib = _lib.load()
    o = _lib.tci_chainstats_options(77)
    assert lib.tci_chainstats_defaults(C.byref(o)) == _lib.TCI_OK and o.max_lag == 0
    assert lib.tci_chainstats_defaults(None) == _lib.TCI_EINVAL
    out = _lib.tci_chainstats_outputs()
    x = np.zeros((20, 1, 1))
    assert lib.tci_chainstats(None, C.byref(o), _lib.ptr(x, _lib._dp), None, 20, 1, 1, None,
                              C.byref(out)) == _lib.TCI_EINVAL
    dopt = _lib.tci_dram_options()
    dout = _lib.tci_dram_outputs()
    assert lib.tci_dram_run_stats(None, C.byref(dopt), 1, None, None, None, None, None, None, None, None, 8,
                                  C.byref(dout), C.byref(o), C.byref(out)) == _lib.TCI_EINVAL
    # the Python wrapper's own checks come before the context is used
    from transcriptioncycleinference_amd.likelihood import Likelihood

    with pytest.raises(ValueError):
        Likelihood.chainstats(object(), np.zeros(5))
