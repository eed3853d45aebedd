"""Marginal densities and histograms without a GPU: the numpy restatement (tests/chaindens_oracle.py) against
its own formulas in numpy.longdouble and against scipy's gaussian_kde within the bounds derived there, its exact
cases and its NaN / padding rules, the MCMCdens schema and result-file round trip, and the argument checks of the C
ABI that come before any device call."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import chaindens_oracle as O

NS = (2, 3, 10, 257, 1000)


def _columns(rng, n):
    for scale in (1e-8, 1.0, 1e6):
        yield f"n={n} scale={scale}", scale * rng.standard_normal(n)
    yield f"near-constant n={n}", 5.0 + 1e-6 * rng.standard_normal(n)   # the hierarchical fit's v


def test_restatement_against_longdouble():
    rng = np.random.default_rng(11)
    for n in NS:
        for where, x in _columns(rng, n):
            for G, s in ((100, 1.0), (7, 0.5)):
                got = O.column(x, G, 20, s)
                bw, dens = O.column_longdouble(x, G, s)
                assert abs(np.longdouble(got["bw"]) - bw) <= O.bw_rel(n) * bw, (where, got["bw"], bw)
                err = np.abs(got["dens"].astype(np.longdouble) - dens).max()
                tol = O.dens_abs(n, got["bw"])
                print(f"{where} G={G}: bw rel {float(abs(got['bw'] - bw) / bw):.2e}, dens err / bound {float(err / tol):.3f}")
                assert err <= tol, (where, G, float(err), float(tol))


def test_restatement_against_scipy_gaussian_kde():
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(12)
    for n in (10, 257, 1000):
        # the three scales; gaussian_kde whitens x by its Cholesky factor before it subtracts, which costs a
        # near-constant column (5 / 1e-6 = 5e6 ulps per unit of z) more than 1e-9: that column is held to the
        # longdouble evaluation above instead
        for where, x in list(_columns(rng, n))[:3]:
            got = O.column(x, 100, 20, 1.0)
            sd = np.std(x, ddof=1)
            kde = stats.gaussian_kde(x, bw_method=got["bw"] / sd)      # kernel sd = factor * sd(x) = bw
            want = kde(got["grid"])
            # gaussian_kde goes through a Cholesky factor and whitened data: an independent statement of the same
            # estimate, not a bit-pinned one; 1e-9 of the peak is the loosest any comparison of dens may be
            peak = O.INV_SQRT_2PI / got["bw"]
            assert np.abs(got["dens"] - want).max() <= 1e-9 * peak, where


def test_exact_cases():
    rng = np.random.default_rng(13)
    x = rng.standard_normal(101)
    c = O.column(x, 100, 20)
    assert c["counts"].dtype == np.int32 and c["counts"].sum() == 101
    assert c["range"].tolist() == [x.min(), x.max()]
    assert c["counts"][-1] >= 1 and c["counts"][0] >= 1                 # xmax lands in the last bin
    assert O.bins_of(np.array([0.0, 1.0, 1.0, 0.5]), 0.0, 1.0, 4).tolist() == [1, 0, 1, 2]
    assert O.bins_of(np.array([0.0, 1.0]), 0.0, 1.0, 1).tolist() == [2]
    g = c["grid"]
    assert len(g) == 100 and g[0] == x.min() - 0.08 * (x.max() - x.min()) and np.all(np.diff(g) > 0)
    assert O.grid_of(1.0, 2.0, 2).tolist() == [1.0 - 0.08, (1.0 - 0.08) + ((2.0 + 0.08) - (1.0 - 0.08))]
    area = np.sum(c["dens"]) * (g[1] - g[0])                              # a density: it integrates to 1
    assert abs(area - 1.0) < 2e-2
    # r == 0: everything in bin 0; a constant column has bw = 0 and a NaN density; range is the value twice
    k = O.column(np.full(9, 0.1), 5, 4)
    assert k["counts"].tolist() == [9, 0, 0, 0] and k["bw"] == 0.0 and np.all(np.isnan(k["dens"]))
    assert k["range"].tolist() == [0.1, 0.1] and k["grid"].tolist() == [0.1] * 5
    # two values, more than three quarters of the rows on one of them: iqr == 0, the bandwidth comes from sd
    two = np.array([2.5] * 9 + [-7.0])
    sd = np.sqrt(np.sum((two - two.mean()) ** 2) / 9)
    assert O.Q.quantiles(two, [0.25, 0.75]).tolist() == [2.5, 2.5]
    assert abs(O.bandwidth(two) - 1.06 * sd * 10 ** -0.2) <= 8 * O.U * O.bandwidth(two)
    assert abs(O.bandwidth(two, 3.0) - 3.0 * O.bandwidth(two)) <= 8 * O.U * O.bandwidth(two, 3.0)
    # the other branch: iqr / 1.34 below sd
    wide = np.concatenate([rng.standard_normal(99), [1e3]])
    q = O.Q.quantiles(wide, [0.25, 0.75])
    assert abs(O.bandwidth(wide) - 1.06 * (q[1] - q[0]) / 1.34 * 100 ** -0.2) <= 8 * O.U * O.bandwidth(wide)


def test_special_columns_and_padding():
    for bad in (np.nan, np.inf, -np.inf):
        c = O.column(np.array([1.0, bad, 2.0]), 4, 3)
        assert np.all(np.isnan(c["range"])) and np.isnan(c["bw"]) and np.all(np.isnan(c["dens"]))
        assert c["counts"].tolist() == [-1, -1, -1]
    z = O.column(np.array([0.0, -0.0, 0.0]), 3, 2)                        # -0 sorts below +0
    assert np.signbit(z["range"][0]) and not np.signbit(z["range"][1]) and z["counts"].tolist() == [3, 0]
    m = O.column(np.array([-0.0, 1.0, 0.0]), 3, 2)
    assert np.signbit(m["range"][0]) and m["range"][1] == 1.0
    ch = np.arange(24.0).reshape(4, 2, 3) ** 2
    ch[2, 0, 1] = np.inf
    t = O.table(ch, s2chain=np.arange(8.0).reshape(4, 2), npar=[3, 2], n_grid=5, n_bins=3)
    assert t["dens"].shape == (2, 5, 3) and t["counts"].shape == (2, 3, 3) and t["range"].shape == (2, 2, 3)
    assert np.all(np.isnan(t["dens"][0, :, 1])) and np.all(t["counts"][0, :, 1] == -1)       # the Inf column
    assert np.all(np.isnan(t["range"][1, :, 2])) and np.all(t["counts"][1, :, 2] == -1)      # the padding
    assert np.isnan(t["bw"][1, 2]) and np.all(np.isfinite(t["dens"][1, :, :2]))
    assert t["counts"][0, :, 0].sum() == 4 and t["s2_counts"].sum(axis=1).tolist() == [4, 4]
    assert t["s2_range"].tolist() == [[0.0, 6.0], [1.0, 7.0]] and np.all(np.isfinite(t["s2_dens"]))
    bare = O.table(ch, npar=[3, 2], n_grid=5, n_bins=3)                   # no s2 chain
    assert np.all(np.isnan(bare["s2_dens"])) and np.all(bare["s2_counts"] == -1) and np.all(np.isnan(bare["s2_bw"]))


def _dens(n=5, G=6, B=4):
    from transcriptioncycleinference_amd.likelihood import ChainDens

    rng = np.random.default_rng(3)
    cd = ChainDens.empty(2, 7 + n + 2, G, B, 1.5)
    cd.n_rows = 301
    P = 7 + n
    cd.range[1, 0, :P], cd.range[1, 1, :P] = -1.0 - np.arange(P), 2.0 + np.arange(P)
    cd.bw[1, :P] = 0.1 + np.arange(P)
    cd.dens[1, :, :P] = rng.random((G, P))
    cd.counts[1, :, :P] = rng.integers(0, 99, (B, P))
    cd.s2_range[1] = [0.5, 9.0]
    cd.s2_bw[1] = 0.25
    cd.s2_dens[1] = rng.random(G)
    cd.s2_counts[1] = rng.integers(0, 99, B)
    return cd


def test_dens_fields_and_dens_entry():
    from transcriptioncycleinference_amd.likelihood import ChainCov, ChainDens, dens_grid
    from transcriptioncycleinference_amd.mcmc import DENS_FIELDS, DramResult, FitResult, dens_entry

    assert DENS_FIELDS == ("grid", "dens", "counts", "range", "bw", "n_rows", "cell_index")
    assert [f.name for f in dataclasses.fields(ChainDens)] == [
        "range", "bw", "dens", "counts", "s2_range", "s2_bw", "s2_dens", "s2_counts", "n_grid", "n_bins", "bw_scale",
        "n_rows", "kernel_ms"]
    # the pins of the earlier reductions still hold
    assert [f.name for f in dataclasses.fields(FitResult)][-1] == "MCMCcov"
    assert [f.name for f in dataclasses.fields(DramResult)][-1] == "cov"
    assert [f.name for f in dataclasses.fields(ChainCov)] == ["mean", "cov", "corr", "n_rows", "kernel_ms"]
    fit_fields = [f.name for f in dataclasses.fields(FitResult)]
    run_fields = [f.name for f in dataclasses.fields(DramResult)]
    assert fit_fields.index("MCMCdens") < fit_fields.index("MCMCquant")
    assert run_fields.index("dens") < run_fields.index("quant")
    cd = _dens(5, 6, 4)
    assert cd.dens.shape == (2, 6, 14) and cd.counts.shape == (2, 4, 14) and cd.counts.dtype == np.int32
    assert cd.s2_dens.shape == (2, 6) and cd.s2_counts.shape == (2, 4) and cd.range.shape == (2, 2, 14)
    o = cd.options()
    assert (o.n_grid, o.n_bins, o.bw_scale) == (6, 4, 1.5)
    g = cd.grid()
    assert g.shape == (2, 6, 14) and np.all(np.isnan(g[0])) and np.all(np.isnan(g[1, :, 12:]))
    for j in range(12):
        assert g[1, :, j].tobytes() == O.grid_of(cd.range[1, 0, j], cd.range[1, 1, j], 6).tobytes()
    assert cd.s2_grid().shape == (2, 6) and cd.s2_grid()[1].tobytes() == O.grid_of(0.5, 9.0, 6).tobytes()
    assert dens_grid(np.array([[1.0], [2.0]]), 2).tolist() == [[1.0 - 0.08], [O.grid_of(1.0, 2.0, 2)[1]]]
    e = dens_entry(cd, 1, 5, 42)
    assert tuple(e) == DENS_FIELDS and e["n_rows"] == 301 and e["cell_index"] == 42
    assert e["grid"].shape == e["dens"].shape == (6, 13) and e["counts"].shape == (4, 13)
    assert e["range"].shape == (2, 13) and e["bw"].shape == (13,) and e["counts"].dtype == np.int32
    assert np.array_equal(e["dens"][:, :12], cd.dens[1, :, :12]) and np.array_equal(e["dens"][:, 12], cd.s2_dens[1])
    assert np.array_equal(e["counts"][:, :12], cd.counts[1, :, :12]) and np.array_equal(e["counts"][:, 12], cd.s2_counts[1])
    assert np.array_equal(e["range"][:, 12], [0.5, 9.0]) and e["bw"][12] == 0.25 and e["bw"][3] == cd.bw[1, 3]
    assert e["grid"][:, :12].tobytes() == np.ascontiguousarray(g[1, :, :12]).tobytes()
    assert e["grid"][:, 12].tobytes() == cd.s2_grid()[1].tobytes()
    for bad in (dict(n_grid=1), dict(n_grid=257), dict(n_bins=0), dict(n_bins=257), dict(bw_scale=0.0),
                dict(bw_scale=-1.0), dict(bw_scale=np.nan), dict(bw_scale=np.inf), dict(n_grid=2.5)):
        with pytest.raises(ValueError):
            ChainDens.empty(1, 8, **bad)


def _fake_fit(with_dens):
    from transcriptioncycleinference_amd.mcmc import CHAIN_FIELDS, FitResult, PLOT_FIELDS, RESULT_FIELDS, dens_entry

    n = 5
    res = {f: (np.arange(n, dtype=float) if f.endswith("_dR") else 1.5) for f in RESULT_FIELDS}
    res["cell_index"], res["ApprovedFits"] = 3, 0
    plot = {f: np.arange(n, dtype=float) for f in PLOT_FIELDS}
    chain = {f: np.zeros((4, n) if f == "dR_chain" else 4) for f in CHAIN_FIELDS}
    dens = [dens_entry(_dens(n), 1, n, 3)] if with_dens else None
    return FitResult("unit", [res], [plot], [chain], np.array([0.3]), 10, 1.0, np.array([2]), MCMCdens=dens)


def test_result_file_round_trip(tmp_path):
    import scipy.io as sio

    from transcriptioncycleinference_amd.mcmc import DENS_FIELDS, save_results

    (tmp_path / "plain").mkdir()
    (tmp_path / "dens").mkdir()
    p0, _ = save_results(_fake_fit(False), str(tmp_path / "plain"), date="01-Jan-2024")
    p1, _ = save_results(_fake_fit(True), str(tmp_path / "dens"), date="01-Jan-2024")
    m0 = sio.loadmat(p0, squeeze_me=True, struct_as_record=False)
    m1 = sio.loadmat(p1, squeeze_me=True, struct_as_record=False)
    names = lambda m: {k for k in m if not k.startswith("__")}  # noqa: E731
    assert names(m0) == {"MCMCresults", "MCMCplot", "DatasetName"}          # the variables of every earlier fit
    assert names(m1) == names(m0) | {"MCMCdens"}
    dv = m1["MCMCdens"]
    want = _fake_fit(True).MCMCdens[0]
    assert tuple(dv._fieldnames) == DENS_FIELDS and dv.n_rows == 301 and dv.cell_index == 3
    for f in DENS_FIELDS[:-2]:
        assert np.array_equal(getattr(dv, f), want[f]), f
    assert dv.counts.dtype == np.int32
    assert tuple(m1["MCMCresults"]._fieldnames) == tuple(m0["MCMCresults"]._fieldnames)


def test_argument_checks_that_need_no_device():
    from transcriptioncycleinference_amd import _lib
    from transcriptioncycleinference_amd.build import build_library

    build_library()
    lib = _lib.load()
    o = _lib.tci_chaindens_options(9, 9, 9.0)
    assert lib.tci_chaindens_defaults(C.byref(o)) == _lib.TCI_OK
    assert (o.n_grid, o.n_bins, o.bw_scale) == (100, 20, 1.0)
    assert lib.tci_chaindens_defaults(None) == _lib.TCI_EINVAL
    out = _lib.tci_chaindens_outputs()
    x = np.zeros((20, 1, 1))
    assert lib.tci_chaindens(None, C.byref(o), _lib.ptr(x, _lib._dp), None, 20, 1, 1, None,
                             C.byref(out)) == _lib.TCI_EINVAL
    names = [f[0] for f in _lib.tci_dram_reductions._fields_]
    assert names == ["sopt", "sout", "copt", "cout", "qopt", "qout", "dopt", "dout"]      # appended after qout
    dopt = _lib.tci_dram_options()
    dout = _lib.tci_dram_outputs()
    for red in (_lib.tci_dram_reductions(), _lib.tci_dram_reductions(dout=C.pointer(out))):   # zeroed: not asked
        assert lib.tci_dram_run_reduced(None, C.byref(dopt), 1, None, None, None, None, None, None, None, None, 8,
                                        C.byref(dout), C.byref(red)) == _lib.TCI_EINVAL
    # the Python wrapper's own checks come before the context is used
    from transcriptioncycleinference_amd.likelihood import Likelihood

    with pytest.raises(ValueError):
        Likelihood.chaindens(object(), np.zeros(5))
    for kw in (dict(n_grid=1), dict(n_bins=300), dict(bw_scale=0.0)):
        with pytest.raises(ValueError):
            Likelihood.chaindens(object(), np.zeros((5, 2)), **kw)
