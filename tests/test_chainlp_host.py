"""The numpy restatement of tci_chainlp (tests/chainlp_oracle.py) on cases worked by hand, the order of the prior sum,
the Python-side argument checks and the sharded fit's packing of MCMClp. CPU only."""
import ctypes as C
import math

import numpy as np
import pytest

import chainlp_oracle as O


def test_three_rows_two_parameters_by_hand():
    # one chain, P = 2: theta rows (1, 2), (3, 2), (1, 0); mu = (1, 0), sig = (2, 1); ss = 8, 2, 4; s2 = 2, 1, 4; nobs 4
    chain = np.array([[[1.0, 2.0]], [[3.0, 2.0]], [[1.0, 0.0]]])
    mu, sig = np.array([[1.0, 0.0]]), np.array([[2.0, 1.0]])
    ss, s2 = np.array([[8.0], [2.0], [4.0]]), np.array([[2.0], [1.0], [4.0]])
    pri, dev, lp = O.traces(chain, s2, ss, [2], [4], mu, sig)
    assert pri[:, 0].tolist() == [4.0, 5.0, 0.0]          # (0/2)^2 + 2^2, (2/2)^2 + 2^2, 0
    want_dev = [8.0 / 2.0 + 4.0 * math.log(O.TWO_PI * 2.0), 2.0 + 4.0 * math.log(O.TWO_PI), 1.0 + 4.0 * math.log(O.TWO_PI * 4.0)]
    assert np.allclose(dev[:, 0], want_dev, rtol=1e-15, atol=0)
    assert np.array_equal(lp[:, 0], -0.5 * (dev[:, 0] + pri[:, 0]))
    tm, sm = O.col_mean(chain[:, 0, :]), O.col_mean(s2)
    assert tm.tolist() == [5.0 / 3.0, 4.0 / 3.0] and sm[0] == 7.0 / 3.0
    r = O.reduce({"ss": ss, "pri": pri, "dev": dev, "lp": lp}, s2, chain, [2], [4], tm[None], sm, np.array([3.0]))
    assert r["ss_min"][0] == 2.0 and r["ss_mean"][0] == 14.0 / 3.0
    assert r["best_row"][0] == 2 and r["lp_best"][0] == lp[2, 0] and r["ss_best"][0] == 4.0 and r["s2_best"][0] == 4.0
    assert r["theta_best"][0].tolist() == [1.0, 0.0]
    dm = ((dev[0, 0] + dev[1, 0]) + dev[2, 0]) / 3.0
    assert r["dev_mean"][0] == dm
    dv = (((dev[0, 0] - dm) ** 2 + (dev[1, 0] - dm) ** 2) + (dev[2, 0] - dm) ** 2) / 2.0
    assert r["dev_var"][0] == dv and r["p_v"][0] == 0.5 * dv
    dh = 3.0 / (7.0 / 3.0) + 4.0 * np.log(O.TWO_PI * (7.0 / 3.0))
    assert r["d_hat"][0] == dh and r["p_d"][0] == dm - dh and r["dic"][0] == dm + (dm - dh)


def test_degenerate_chains():
    chain = np.zeros((1, 2, 3))
    one = {f: np.ones((1, 2)) for f in ("ss", "pri", "dev", "lp")}
    r = O.reduce(one, np.ones((1, 2)), chain, [3, 2], [4, 4], np.zeros((2, 3)), np.ones(2), np.ones(2))
    assert np.all(np.isnan(r["dev_var"])) and np.all(np.isnan(r["p_v"])) and np.all(r["best_row"] == 0)   # n = 1
    assert np.isnan(r["theta_best"][1, 2]) and np.isnan(r["theta_mean"][1, 2]) and r["theta_best"][0, 2] == 0.0
    for f, v in (("ss", np.inf), ("pri", np.nan), ("dev", -np.inf)):    # a non-finite trace value: NaN and -1
        tr = {k: np.ones((5, 2)) for k in ("ss", "pri", "dev", "lp")}
        tr[f][3, 1] = v
        r = O.reduce(tr, np.ones((5, 2)), np.zeros((5, 2, 3)), [3, 3], [4, 4], np.zeros((2, 3)), np.ones(2), np.ones(2))
        assert all(np.isnan(r[k][1]) and np.isfinite(r[k][0]) for k in O.SCALARS)
        assert r["best_row"].tolist() == [0, -1] and np.all(np.isnan(r["theta_best"][1])) and np.all(np.isnan(r["theta_mean"][1]))
    lp = np.array([1.0, 3.0, 3.0, 2.0, 3.0])[:, None]               # ties: the first of the largest
    tr = {"ss": np.ones((5, 1)), "pri": np.ones((5, 1)), "dev": np.ones((5, 1)), "lp": lp}
    assert O.reduce(tr, np.ones((5, 1)), np.zeros((5, 1, 2)), [2], [4], np.zeros((1, 2)), np.ones(1), np.ones(1))["best_row"][0] == 1
    assert O.pri(np.array([1.0, 5.0]), np.array([0.0, 0.0]), np.array([np.inf, 1.0])) == 25.0   # sig = +Inf: exactly 0
    assert np.isnan(O.pri(np.array([np.nan, 5.0]), np.zeros(2), np.array([np.inf, 1.0])))


def test_the_64_partial_order_is_not_the_plain_order():
    """P = 130: lane 1 adds j = 1, 65, 129 before it meets lane 0. With term 0 = 1 and terms 1, 65, 129 = 2^-54 the
    plain ascending sum loses every small term (1 + 2^-54 rounds to 1), while lane 1's partial 3 x 2^-54 survives into
    the sum of partials (it rounds up to one ulp of 1)."""
    P = 130
    theta, mu, sig = np.zeros(P), np.zeros(P), np.ones(P)
    theta[0] = 1.0
    theta[[1, 65, 129]] = 2.0 ** -27     # squared: 2^-54
    t = O.pri_terms(theta, mu, sig)
    assert t[0] == 1.0 and np.all(t[[1, 65, 129]] == 2.0 ** -54)
    a, b = O.pri(theta, mu, sig), O.pri_plain(theta, mu, sig)
    assert b == 1.0 and a == 1.0 + 2.0 ** -52 and a != b


def test_segment_sums_follow_n_alone():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((513, 2)) * 10.0 ** rng.uniform(-3, 3, (513, 2))
    want = ((0.0 + sum_in_order(x[:256])) + sum_in_order(x[256:512])) + (0.0 + x[512])
    assert np.array_equal(O.seg_sum(x), want)
    assert not np.array_equal(want, sum_in_order(x))    # the segments are not the plain running sum
    m = O.col_mean(np.stack([np.full(7, 0.1), np.arange(7.0), np.array([1, 2, np.inf, 4, 5, 6, 7.0])], axis=1))
    assert m[0] == 0.1 and m[1] == 3.0 and np.isnan(m[2])


def sum_in_order(x):
    acc = np.zeros(x.shape[1:])
    for row in x:
        acc = acc + row
    return acc


def test_the_bound_stays_under_the_parity_cap():
    """At the tests' inputs (s2 from 1e-2 to 1e4, 2 N up to 1,200, ss / s2 up to 1e6) the header's bound is below
    1e-10 max(1, |value|)."""
    for s2 in (1e-2, 1.0, 1e4):
        for nobs in (4, 246, 1200):
            for ss in (0.0, s2, 1e6 * s2):
                d = float(O.dev(ss, s2, nobs))
                lp = float(O.lp(d, 100.0))
                e_dev, e_lp = O.bounds(ss, s2, nobs, d, lp)
                assert e_dev <= 1e-10 * max(1.0, abs(d)) and e_lp <= 1e-10 * max(1.0, abs(lp))


def test_arguments_are_checked_without_a_gpu():
    from transcriptioncycleinference_amd import _lib, mcmc
    from transcriptioncycleinference_amd.likelihood import ChainLp

    e = ChainLp.empty(5, 2, 9)
    assert e.ss.shape == (5, 2) and e.theta_best.shape == (2, 9) and e.best_row.dtype == np.int64
    assert np.all(e.best_row == -1) and e.options().flags == 0
    out = e.to_c()
    assert [f for f, _ in out._fields_][:4] == list(_lib.CHAINLP_TRACES) and _lib.CHAINLP_SCALARS == O.SCALARS
    assert "MCMClp" in mcmc.FitResult.__dataclass_fields__ and mcmc.LP_FIELDS[:2] == ("ss_min", "ss_mean")
    dopt, dout, red = _lib.tci_dram_options(), _lib.tci_dram_outputs(), _lib.tci_dram_reductions()
    run = lambda ctx, lout: _lib.load().tci_dram_run_lp(ctx, C.byref(dopt), 1, None, None, None, None, None, None, None,  # noqa: E731
                                                       None, 8, C.byref(dout), C.byref(red), None, 0, None, None, None,
                                                       None, None, lout)
    assert run(None, C.byref(out)) == _lib.TCI_EINVAL
    with pytest.raises(ValueError):   # MCMClp needs the kept rows (checked before the library is touched)
        mcmc.fit(None, n_steps=10, n_burn=1, thin=0, logpost=True)
    lib = _lib.load()
    o = _lib.tci_chainlp_options(7)
    assert lib.tci_chainlp_defaults(C.byref(o)) == 0 and o.flags == 0
    assert lib.tci_chainlp_defaults(None) == _lib.TCI_EINVAL
    assert lib.tci_chainlp(None, None, None, None, 1, 1, 9, None, None, None, None) == _lib.TCI_EINVAL


def entry(M, n, cell_index, seed):
    from transcriptioncycleinference_amd import mcmc
    from transcriptioncycleinference_amd.likelihood import ChainLp

    rng = np.random.default_rng(seed)
    K, rows = 2, 4
    clp = ChainLp.empty(rows, K * M, 7 + n + 1)
    for f in mcmc.LP_SCALARS + ("ss", "lp", "theta_best"):
        getattr(clp, f)[...] = rng.standard_normal(getattr(clp, f).shape)
    clp.best_row[:] = rng.integers(0, rows, K * M)
    clp.n_rows = rows
    grp = {f: rng.standard_normal(K) for f in ("lp_rhat", "lp_rhat_split", "lp_ess", "lp_mcse")} if M > 1 else None
    return mcmc.lp_entry(clp, 1, n, cell_index, K, M, grp), clp


@pytest.mark.parametrize("M", [1, 3])
def test_lp_entries_and_their_packing(M):
    from transcriptioncycleinference_amd import mcmc, parallel

    (a, clp), (b, _) = entry(M, 5, 12, 1), entry(M, 3, 4, 2)
    assert set(a) == set(mcmc.LP_FIELDS + (mcmc.LP_GROUP_FIELDS if M > 1 else ()))
    if M == 1:
        assert a["ss"].shape == (4,) and a["best_dR"].shape == (5,) and isinstance(a["dic"], float)
        assert a["dic"] == clp.dic[1] and a["best_v"] == clp.theta_best[1, 0] and a["best_row"] == clp.best_row[1]
    else:
        assert a["ss"].shape == (M, 4) and a["best_dR"].shape == (M, 5) and a["dic"].shape == (M,)
        assert np.array_equal(a["dic"], clp.dic[[1, 3, 5]]) and np.array_equal(a["lp"][2], clp.lp[:, 5])
        assert a["ss_gap"] == np.max(a["ss_mean"]) - np.min(a["ss_mean"])
        assert a["best_replicate"] == int(np.argmax(a["lp_best"]))
    assert parallel.lp_rows(240, 41, 1) == 200 and parallel.lp_rows(200000, 100000, 100) == 1000
    assert parallel.lp_rows(200000, 10000, 1) == 190001 and parallel.lp_rows(10, 0, 3) == 4 and parallel.lp_rows(10, 5, 0) == 0
    rows = parallel.pack_lp([a, b], M, 6, 4)
    assert rows.shape == (2, parallel.lp_width(M, 6, 4))
    with pytest.raises(ValueError):
        parallel.pack_lp([a], M, 6, 5)
    back = parallel.unpack_lp(rows[::-1])
    assert [e["cell_index"] for e in back] == [4, 12]
    for want, got in ((b, back[0]), (a, back[1])):
        assert set(got) == set(want)
        for f in want:
            assert np.array_equal(np.asarray(got[f]), np.asarray(want[f])), f
            assert np.shape(got[f]) == np.shape(want[f]) and type(got[f]) is type(want[f]), f
