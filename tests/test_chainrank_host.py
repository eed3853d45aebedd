"""The restatement of tci_chainrank (chainrank_oracle) on the CPU: its ranks are scipy's average ranks and its scores
scipy's ndtri to a few ulp, the stated special cases hold, the statistical cases the GPU test asserts hold for the
oracle with the same seeds, and the bindings check their arguments."""
import ctypes as C

import numpy as np
import pytest

import chainrank_oracle as O


def sanity_chains(kind, seed=11, n=500, M=4):
    """The host-generated chains of the statistical cases, [n, M, 1]; shared with test_chainrank_gpu."""
    rng = np.random.default_rng(seed)
    if kind == "iid":
        x = rng.standard_normal((n, M))
    elif kind == "scales":
        x = rng.standard_normal((n, M)) * np.array([1.0, 1.0, 1.0, 3.0])
    else:
        x = rng.standard_cauchy((n, M))
    return np.ascontiguousarray(x[:, :, None])


def test_ranks_are_scipys_average_ranks_and_z_is_ndtri_to_a_few_ulp():
    stats = pytest.importorskip("scipy.stats")
    special = pytest.importorskip("scipy.special")
    rng = np.random.default_rng(3)
    worst = 0.0
    for N in (2, 3, 5, 64, 257, 4000):
        for ties in (False, True):
            x = rng.standard_normal(N)
            if ties:
                x = np.round(x, 1) + 0.0  # many repeated values; -0 made +0, which scipy ties and the key order does not
            r2 = O.rank2(x)
            assert np.array_equal(r2, np.rint(2 * stats.rankdata(x, method="average")).astype(np.int64))
            z, p = O.scores(x)
            worst = max(worst, float(np.max(O.ulp_diff(z, special.ndtri(p)))))
    print(f"largest |z - ndtri(p)|: {worst:.1f} ulp")
    # measured 5.0 ulp on this data; both are rational approximations good to about 1e-16 relative
    assert worst <= 8.0


def test_special_cases():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((40, 3, 2))
    t = O.table(x)
    assert np.all(np.isfinite(t["rhat_rank"][:, :2])) and np.all(np.isfinite(t["ess_tail"][:, :2]))
    assert np.all(t["window_bulk"][:, :2] > 0) and np.all(t["window_bulk"][:, 2] == -1)  # no s2 chain: NaN / -1
    # ties take the average rank: two equal values share one z
    y = x.copy()
    y[5, 0, 0] = y[9, 2, 0]
    t = O.table(y, stats=False)
    assert t["z"][5, 0, 0] == t["z"][9, 2, 0] and t["p"][5, 0, 0] == t["p"][9, 2, 0]
    # -0 sorts below +0 and they do not tie
    zz = np.zeros((4, 1, 1))
    zz[1, 0, 0] = -0.0
    t = O.table(zz, stats=False)
    assert t["z"][1, 0, 0] < t["z"][0, 0, 0] == t["z"][2, 0, 0]
    # a constant column: every R2 = N + 1, p = 0.5, z = 0; rhat and ess NaN
    const = np.full((40, 3, 1), 2.5)
    t = O.table(const)
    assert np.all(t["p"][:, :, 0] == 0.5) and np.all(t["z"][:, :, 0] == 0.0)
    assert np.isnan(t["rhat_rank"][0, 0]) and np.isnan(t["ess_bulk"][0, 0]) and np.isnan(t["ess_tail"][0, 0])
    assert t["q"][0, 1, 0] == 2.5
    # a non-finite entry: everything NaN, every window -1
    for v in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[7, 2, 0] = v
        t = O.table(y)
        for k in ("rhat_bulk", "rhat_folded", "rhat_rank", "ess_bulk", "tau_bulk", "ess_tail_lo", "ess_tail_hi", "ess_tail"):
            assert np.isnan(t[k][0, 0]) and np.isfinite(t[k][0, 1]), k
        assert np.all(np.isnan(t["q"][0, :, 0])) and np.all(np.isnan(t["z"][:, :, 0]))
        assert t["window_bulk"][0, 0] == t["window_tail_lo"][0, 0] == t["window_tail_hi"][0, 0] == -1
    # M = 1: the two halves of the one chain
    t = O.table(x[:, :1])
    assert np.all(np.isfinite(t["rhat_rank"][:, :2])) and np.all(np.isfinite(t["ess_bulk"][:, :2]))
    # n < 4: no split sequence; quantiles and scores are defined
    for n in (1, 2, 3):
        t = O.table(x[:n])
        assert np.all(np.isnan(t["rhat_rank"])) and np.all(np.isnan(t["ess_bulk"])) and np.all(t["window_bulk"][:, :2] == 0)
        assert np.all(np.isfinite(t["q"][:, :, :2])) and np.all(np.isfinite(t["z"][:, :, :2]))
    # padding and a group id no chain carries
    t = O.table(x, npar=[1, 1, 1], group=[2, 0, 2])
    assert np.all(np.isnan(t["rhat_rank"][1])) and np.all(np.isnan(t["rhat_rank"][:, 1])) and t["q"].shape == (3, 3, 3)
    assert np.all(np.isfinite(t["rhat_rank"][[0, 2], 0]))


def test_the_statistical_cases_hold_for_the_oracle():
    import chainrhat_oracle as R

    t = O.table(sanity_chains("iid"))
    print("iid", t["rhat_rank"][0, 0], t["ess_bulk"][0, 0], t["ess_tail"][0, 0])
    assert t["rhat_rank"][0, 0] < 1.05 and 1000 <= t["ess_bulk"][0, 0] <= 4000
    x = sanity_chains("scales")
    t = O.table(x)
    classic = R.table(x)["rhat"][0, 0]
    print("scales", t["rhat_bulk"][0, 0], t["rhat_folded"][0, 0], classic)
    assert t["rhat_folded"][0, 0] > 1.1 and t["rhat_folded"][0, 0] > t["rhat_bulk"][0, 0] + 0.05 and classic < 1.05
    t = O.table(sanity_chains("cauchy"))
    print("cauchy", t["rhat_rank"][0, 0], t["ess_bulk"][0, 0], t["ess_tail"][0, 0])
    assert t["rhat_rank"][0, 0] < 1.05 and 500 <= t["ess_bulk"][0, 0] <= 4000 and 100 <= t["ess_tail"][0, 0] <= 4000


def test_arguments_are_checked_without_a_gpu():
    from transcriptioncycleinference_amd import _lib
    from transcriptioncycleinference_amd.likelihood import ChainRank

    for bad in ({"tail": (0.0, 0.9)}, {"tail": (0.6, 0.5)}, {"tail": (0.1, 1.0)}, {"max_lag": -1}, {"max_lag": 1.5},
                {"probs": (1.5,)}, {"probs": ()}, {"probs": (0.5,) * 17}):
        with pytest.raises(ValueError):
            ChainRank.empty(2, 3, **bad)
    k = ChainRank.empty(2, 3, probs=(0.1, 0.9), tail=(0.2, 0.8), max_lag=7, scores=(5, 4, True))
    assert k.q.shape == (2, 2, 3) and k.q_tail.shape == (2, 2, 3) and k.s2_q.shape == (2, 2) and k.rhat_rank.shape == (2, 3)
    assert k.window_bulk.dtype == np.int32 and np.all(k.s2_window_tail_hi == -1) and k.z.shape == (5, 4, 3)
    assert k.s2_z_folded.shape == (5, 4)
    o = k.options()
    assert (o.nq, o.probs[1], o.tail_lo, o.tail_hi, o.max_lag, o.flags) == (2, 0.9, 0.2, 0.8, 7, 0)
    lib = _lib.load()
    d = _lib.tci_chainrank_options()
    assert lib.tci_chainrank_defaults(None) == _lib.TCI_EINVAL and lib.tci_chainrank_defaults(C.byref(d)) == _lib.TCI_OK
    assert (d.nq, list(d.probs)[:3], d.tail_lo, d.tail_hi, d.max_lag, d.flags) == (3, [0.025, 0.5, 0.975], 0.05, 0.95, 0, 0)
    cap = lib.tci_chainrank_lds_cap()
    assert cap >= 6464 and cap & (cap - 1) == 0  # both sampler shapes sort in LDS
    out = _lib.tci_chainrank_outputs()
    x = np.zeros((4, 1, 1))
    assert lib.tci_chainrank(None, None, _lib.ptr(x, _lib._dp), None, 4, 1, 1, None, None, 1, C.byref(out)) == _lib.TCI_EINVAL
    assert lib.tci_dram_run_rank(None, None, 1, *(None,) * 8, 8, *(None,) * 3, 1, *(None,) * 6) == _lib.TCI_EINVAL
    assert lib.tci_demc_run_rank(None, None, None, 8, None, 1, 4, *(None,) * 13) == _lib.TCI_EINVAL
