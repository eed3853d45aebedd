"""The group reduction (tci_chainrhat) without a device: the FP64 restatement of include/tci.h against its longdouble
twin within the derived bound on every fixture the device tests use, the identities of the definition, the Python
types, the result file and the argument checks that come before any device work."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import chainrhat_oracle as O


@pytest.fixture(scope="module")
def cases():
    return O.all_cases()


@pytest.fixture(scope="module")
def refs(cases):
    return {c["name"]: O.table(c["chain"], c["s2"], c["npar"], c["group"], dtype=O.LD) for c in cases}


def test_restatement_within_the_bound_in_every_sum_order(cases, refs):
    """The reference alone meets the bound: forward, reversed and pairwise sums. The bound itself is below 1e-9 on
    every fixture but the offset one (a wider one would say the fixture, or the derivation, is wrong)."""
    for c in cases:
        ref = refs[c["name"]]
        for order in O.ORDERS:
            got = O.table(c["chain"], c["s2"], c["npar"], c["group"], dtype=np.float64, order=order)
            worst, widest = O.check(got, ref, c["n"], where=(c["name"], order))
            assert max(worst.values()) <= 1.0
        print(f"{c['name']}: widest bound rhat {widest['rhat']:.3e} split {widest['rhat_split']:.3e}")
        if c["name"] != "offset":
            assert widest["rhat"] < 1e-9 and widest["rhat_split"] < 1e-9, (c["name"], widest)
    ref = refs["offset"]
    b = O.bounds(ref, 1000)
    print(f"offset fixture: rhat {float(ref['rhat'][0, 0]):.12f}, bound {b['rhat'][0, 0]:.3e} "
          f"(split {b['rhat_split'][0, 0]:.3e})")
    assert 1e-12 < b["rhat"][0, 0] < 1e-8       # the cancellation term: five orders above a centred column's


def test_identities():
    rng = np.random.default_rng(3)
    # identical chains: exactly sqrt((L - 1) / L), for every M the sweep uses
    for M in (2, 3, 4, 7):
        for n in (31, 256, 1000):
            one = 0.3 + rng.standard_normal((n, 1, 5))
            t = O.table(np.repeat(one, M, axis=1))
            assert np.array_equal(t["rhat"][0, :5], np.full(5, np.sqrt(np.float64(n - 1) / np.float64(n))))
            assert np.array_equal(t["pooled_mean"][0, :5], O.table(one)["pooled_mean"][0, :5])
    # pooled_std is the std(., 1) of the stacked rows
    x = 2.0 + rng.standard_normal((257, 4, 3)) * np.array([1e-3, 1.0, 50.0])
    ref = O.table(x, dtype=O.LD)
    got = O.table(x)
    stacked = x.reshape(-1, 3).astype(O.LD)
    b = O.bounds(ref, 257)
    assert np.all(np.abs(got["pooled_std"][0, :3] - np.std(stacked, axis=0)) <= b["pooled_std"][0, :3])
    assert np.all(np.abs(got["pooled_mean"][0, :3] - np.mean(stacked, axis=0)) <= b["pooled_mean"][0, :3])
    # one chain: no classic factor, a finite split one
    t = O.table(x[:, :1])
    assert np.all(np.isnan(t["rhat"])) and np.all(np.isfinite(t["rhat_split"][0, :3]))
    assert np.all(np.isfinite(t["pooled_std"][0, :3]))
    # halves of one row: no split factor
    for n in (2, 3):
        t = O.table(x[:n])
        assert np.all(np.isnan(t["rhat_split"])) and np.all(np.isfinite(t["rhat"][0, :3]))
    assert np.all(np.isfinite(O.table(x[:4])["rhat_split"][0, :3]))
    # an odd n: the middle row belongs to no half
    y = x[:5].copy()
    z = y.copy()
    z[2] += 100.0
    assert O.table(y)["rhat_split"].tobytes() == O.table(z)["rhat_split"].tobytes()
    assert O.table(y)["rhat"].tobytes() != O.table(z)["rhat"].tobytes()


def test_special_columns(refs):
    r = refs["special"]
    assert np.isfinite(r["rhat"][0, 0]) and np.isfinite(r["rhat"][0, 7]) and np.isfinite(r["rhat"][0, 8])
    assert np.isnan(r["rhat"][0, 1]) and r["pooled_mean"][0, 1] == 2.5 and r["pooled_std"][0, 1] == 0.0
    assert np.isfinite(r["rhat"][0, 2])
    assert np.isposinf(r["rhat"][0, 3]) and np.isposinf(r["rhat_split"][0, 3])
    for j in (4, 5):
        assert all(np.isnan(r[k][0, j]) for k in O.OUTPUTS)
    assert np.float64(r["rhat"][0, 6]) == np.sqrt(np.float64(299) / np.float64(300))


def _rhat(n=5, M=3):
    from transcriptioncycleinference_amd.likelihood import ChainRhat

    cr = ChainRhat.empty(2, 14)
    rng = np.random.default_rng(8)
    for k in O.OUTPUTS:
        getattr(cr, k)[1, :7 + n] = 1.0 + rng.random(7 + n)
        getattr(cr, "s2_" + k)[1] = 1.0 + rng.random()
    cr.rhat[1, 3] = 1.75
    cr.n_rows = 301
    return cr


def test_rhat_fields_and_rhat_entry():
    from transcriptioncycleinference_amd import _lib
    from transcriptioncycleinference_amd.likelihood import ChainRhat
    from transcriptioncycleinference_amd.mcmc import RHAT_FIELDS, DramResult, FitPlan, FitResult, rhat_entry

    assert RHAT_FIELDS == ("rhat", "rhat_split", "pooled_mean", "pooled_std", "mean_rep", "accept_rep", "rhat_max",
                           "n_rows", "n_chains", "cell_index")
    assert [f.name for f in dataclasses.fields(ChainRhat)] == [
        "rhat", "rhat_split", "pooled_mean", "pooled_std", "s2_rhat", "s2_rhat_split", "s2_pooled_mean",
        "s2_pooled_std", "n_rows", "kernel_ms"]
    assert [f[0] for f in _lib.tci_chainrhat_outputs._fields_] == [f.name for f in dataclasses.fields(ChainRhat)]
    assert [f[0] for f in _lib.tci_chainrhat_options._fields_] == ["flags"]
    fit_fields = [f.name for f in dataclasses.fields(FitResult)]
    run_fields = [f.name for f in dataclasses.fields(DramResult)]
    assert fit_fields.index("MCMCrhat") + 1 == fit_fields.index("MCMCdens") and fit_fields[-1] == "MCMCcov"
    assert run_fields.index("rhat") + 1 == run_fields.index("dens") and run_fields[-1] == "cov"
    assert [f.name for f in dataclasses.fields(FitPlan)][-1] == "replicates"
    cr = _rhat()
    assert cr.rhat.shape == (2, 14) and cr.s2_pooled_std.shape == (2,) and np.all(np.isnan(cr.rhat[0]))
    assert cr.options().flags == 0
    mean_rep, acc = np.arange(3 * 14, dtype=float).reshape(3, 14), np.array([0.2, 0.3, 0.4])
    e = rhat_entry(cr, 1, 5, 42, mean_rep, acc)
    assert tuple(e) == RHAT_FIELDS and e["n_rows"] == 301 and e["cell_index"] == 42 and e["n_chains"] == 3
    for k in O.OUTPUTS:
        assert e[k].shape == (13,) and np.array_equal(e[k][:12], getattr(cr, k)[1, :12])
        assert e[k][12] == getattr(cr, "s2_" + k)[1]
    assert e["mean_rep"].shape == (3, 12) and np.array_equal(e["mean_rep"], mean_rep[:, :12])
    assert np.array_equal(e["accept_rep"], acc) and e["rhat_max"] == max(e["rhat"].max(), e["rhat_split"].max())
    assert np.isnan(rhat_entry(cr, 0, 5, 1, mean_rep, acc)["rhat_max"])


def _fake_fit(with_rhat):
    from transcriptioncycleinference_amd.mcmc import CHAIN_FIELDS, FitResult, PLOT_FIELDS, RESULT_FIELDS, rhat_entry

    n = 5
    res = {f: (np.arange(n, dtype=float) if f.endswith("_dR") else 1.5) for f in RESULT_FIELDS}
    res["cell_index"], res["ApprovedFits"] = 3, 0
    plot = {f: np.arange(n, dtype=float) for f in PLOT_FIELDS}
    chain = {f: np.zeros((4, n) if f == "dR_chain" else 4) for f in CHAIN_FIELDS}
    rh = [rhat_entry(_rhat(n), 1, n, 3, np.ones((3, 14)), np.array([0.2, 0.3, 0.4]))] if with_rhat else None
    return FitResult("unit", [res], [plot], [chain], np.array([0.3]), 10, 1.0, np.array([2]), MCMCrhat=rh)


def test_result_file_round_trip(tmp_path):
    import scipy.io as sio

    from transcriptioncycleinference_amd.mcmc import RHAT_FIELDS, save_results

    (tmp_path / "plain").mkdir()
    (tmp_path / "rhat").mkdir()
    p0, _ = save_results(_fake_fit(False), str(tmp_path / "plain"), date="01-Jan-2024")
    p1, _ = save_results(_fake_fit(True), str(tmp_path / "rhat"), date="01-Jan-2024")
    m0 = sio.loadmat(p0, squeeze_me=True, struct_as_record=False)
    m1 = sio.loadmat(p1, squeeze_me=True, struct_as_record=False)
    names = lambda m: {k for k in m if not k.startswith("__")}  # noqa: E731
    assert names(m0) == {"MCMCresults", "MCMCplot", "DatasetName"}          # the variables of every earlier fit
    assert names(m1) == names(m0) | {"MCMCrhat"}
    rv = m1["MCMCrhat"]
    want = _fake_fit(True).MCMCrhat[0]
    assert tuple(rv._fieldnames) == RHAT_FIELDS and rv.n_rows == 301 and rv.cell_index == 3 and rv.n_chains == 3
    for f in RHAT_FIELDS[:6]:
        assert np.array_equal(getattr(rv, f), want[f]), f
    assert rv.rhat_max == want["rhat_max"]
    assert tuple(m1["MCMCresults"]._fieldnames) == tuple(m0["MCMCresults"]._fieldnames)


def test_replicate_keys():
    """A chain's key reaches the generator modulo 2^32 (include/tci.h): the replicates' keys are distinct there, and
    replicate 0's is the cell index, the one-chain fit's key."""
    from transcriptioncycleinference_amd.mcmc import MAX_REPLICATES, REPLICATE_KEY_STRIDE, replicate_keys

    g = np.array([0, 7, 298, 9_999, REPLICATE_KEY_STRIDE - 1])
    for M in (1, 2, 4, MAX_REPLICATES):
        k = replicate_keys(g, M)
        assert k.dtype == np.int64 and k.shape == (M * len(g),) and np.array_equal(k[:len(g)], g)
        assert len(np.unique(k % 2**32)) == len(k) and k.max() < 2**32
        assert np.array_equal(k.reshape(M, -1) - g, np.arange(M)[:, None] * REPLICATE_KEY_STRIDE * np.ones(len(g), np.int64))
    assert np.array_equal(replicate_keys([2**40], 1), [2**40])          # one chain per cell: any index, as before
    for bad in (([REPLICATE_KEY_STRIDE], 2), ([-1], 2), ([0], MAX_REPLICATES + 1), ([0], 0), ([0], 1.5)):
        with pytest.raises(ValueError):
            replicate_keys(*bad)


def test_argument_checks_that_need_no_device():
    """What is refused before any device work. The C ABI reports its refusals through a context, and a context needs a
    device: without one only the null-context refusal of the entry points can be reached, and the refusals of
    flags != 0, a group id out of range and mixed npar in the C layer are asserted in the device tests
    (test_chainrhat_gpu.py::test_bad_arguments_are_refused). Here: the null context, the defaults, and the Python
    wrappers' own checks of the same arguments, which come before the context is used."""
    from transcriptioncycleinference_amd import _lib
    from transcriptioncycleinference_amd.build import build_library
    from transcriptioncycleinference_amd.likelihood import Likelihood, rhat_groups
    from transcriptioncycleinference_amd.mcmc import fit, plan_fit

    build_library()
    lib = _lib.load()
    o = _lib.tci_chainrhat_options(9)
    assert lib.tci_chainrhat_defaults(C.byref(o)) == _lib.TCI_OK and o.flags == 0
    assert lib.tci_chainrhat_defaults(None) == _lib.TCI_EINVAL
    out = _lib.tci_chainrhat_outputs()
    x = np.zeros((20, 2, 1))
    assert lib.tci_chainrhat(None, C.byref(o), _lib.ptr(x, _lib._dp), None, 20, 2, 1, None, None, 1,
                             C.byref(out)) == _lib.TCI_EINVAL
    dopt, dout = _lib.tci_dram_options(), _lib.tci_dram_outputs()
    assert lib.tci_dram_run_rhat(None, C.byref(dopt), 2, None, None, None, None, None, None, None, None, 8,
                                 C.byref(dout), None, None, 1, None, C.byref(out)) == _lib.TCI_EINVAL
    # the reductions struct is the one the earlier entry point takes: the group reduction is not a field of it
    assert [f[0] for f in _lib.tci_dram_reductions._fields_] == ["sopt", "sout", "copt", "cout", "qopt", "qout", "dopt",
                                                                 "dout"]
    # the Python wrapper's own checks come before the context is used
    with pytest.raises(ValueError):
        Likelihood.chainrhat(object(), np.zeros(5))
    for bad in ([0, 1, 3], [0, -2, 0], [0, 1], [0.0, 1.0, 0.0]):
        with pytest.raises(ValueError):
            Likelihood.chainrhat(object(), np.zeros((5, 3, 2)), group=np.array(bad))
    with pytest.raises(ValueError, match="group 1 .* npar"):
        Likelihood.chainrhat(object(), np.zeros((5, 3, 2)), npar=[2, 1, 2], group=np.array([1, 1, 1]))
    g, ng = rhat_groups(np.array([2, -1, 0, 2]), 4, [1, 9, 3, 1])
    assert g.dtype == np.int32 and ng == 3 and rhat_groups(None, 3)[1] == 1
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="replicates"):
            fit(object(), replicates=bad)
        with pytest.raises(ValueError, match="replicates"):
            plan_fit(None, [], 0, replicates=bad)
    with pytest.raises(ValueError, match="thin"):
        fit(object(), replicates=2)                      # MCMCrhat needs the kept rows
    with pytest.raises(ValueError, match="thin"):
        fit(object(), rhat=True, thin=0)


def test_replicate_plan(cells):
    """Replicate 0 of every cell is the one-chain plan bit for bit; the others start elsewhere, inside the same
    bounds, with the cell's own priors and proposal scales."""
    from transcriptioncycleinference_amd.mcmc import plan_fit

    ids = [5, 0, 17]
    one = plan_fit(cells, ids, 11, cell_offset=100)
    rep = plan_fit(cells, ids, 11, cell_offset=100, replicates=4)
    K = len(ids)
    assert one.replicates == 1 and rep.replicates == 4 and rep.cells == one.cells and rep.approved == one.approved
    assert rep.x0.shape == (4 * K, one.x0.shape[1])
    for f in ("x0", "lower", "upper", "prior_mu", "prior_sig", "qcov_diag"):
        assert np.ascontiguousarray(getattr(rep, f)[:K]).tobytes() == getattr(one, f).tobytes(), f
    for r in range(1, 4):
        for f in ("lower", "upper", "prior_mu", "prior_sig", "qcov_diag"):
            assert np.array_equal(getattr(rep, f)[r * K:(r + 1) * K], getattr(one, f)), (r, f)
        for k, c in enumerate(ids):
            P = 7 + int(cells.lengths[c])
            a = rep.x0[r * K + k, :P]
            assert np.all(a >= rep.lower[k, :P]) and np.all(a <= rep.upper[k, :P])
            for r2 in range(r):
                assert not np.array_equal(a, rep.x0[r2 * K + k, :P])
            want = plan_fit(cells, [c], 11, cell_offset=100, replicates=r + 1).x0[r, :P]   # keyed by cell, not position
            assert np.array_equal(a, want)
    # a hierarchical fit: every replicate keeps the cell's own v0
    v0 = {100 + c + 1: 4.0 + 0.1 * k for k, c in enumerate(ids)}
    hier = plan_fit(cells, ids, 11, v0=v0, cell_offset=100, replicates=3)
    for r in range(3):
        assert np.array_equal(hier.lower[r * K:(r + 1) * K, 0], hier.lower[:K, 0])
        assert np.all(np.abs(hier.x0[r * K:(r + 1) * K, 0] - np.array([4.0, 4.1, 4.2])) <= 1e-5)
