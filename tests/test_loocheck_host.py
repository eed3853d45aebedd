"""The numpy restatement of tci_loocheck (tests/loocheck_oracle.py) against closed forms, the tail length, and the
argument checks of fit(..., stack=...). No device."""
import numpy as np
import pytest

import loocheck_oracle as LO


def test_tail_length():
    assert LO.tail_count(32) == (6, 32)
    assert 225 // 5 == 45 and 3 * 15 == 45 and LO.tail_count(225)[0] == 45      # both terms of M
    assert LO.tail_count(4096) == (192, 43)
    assert LO.tail_count(500) == (68, 38)
    for S in (31, 4097):
        with pytest.raises(ValueError):
            LO.tail_count(S)
    from transcriptioncycleinference_amd.likelihood import loocheck_tail, loocheck_threshold

    for S in (32, 64, 65, 224, 225, 226, 500, 4096):
        assert loocheck_tail(S) == LO.tail_count(S)
        assert loocheck_threshold(S) == LO.default_threshold(S)
    assert LO.default_threshold(4096) == 0.7 and LO.default_threshold(32) < 0.34


def test_key_order():
    x = np.array([-np.inf, -1.0, -0.0, 0.0, 5e-324, 1.0, np.inf, np.nan])
    k = LO.to_key(x)
    assert np.all(k[1:] > k[:-1])


@pytest.mark.parametrize("S", [32, 65, 500])
def test_identical_rows_are_degenerate(S):
    """Identical sample rows: every ratio is equal, x_M = 0, khat = +Inf, the weights stay equal and the LOO density is
    the posterior predictive one."""
    rng = np.random.default_rng(S)
    N = 7
    sim = np.repeat(rng.normal(5, 1, (1, N)), S, axis=0)
    y = rng.normal(5, 1, N)
    got = LO.pointwise(sim, y, np.full(S, 0.8))
    assert np.all(np.isposinf(got["khat_i"]))
    assert np.all(np.abs(got["p_loo_i"]) <= 1e-12 * np.maximum(1.0, np.abs(got["lppd_i"])))
    assert np.all(np.abs(got["elpd_loo_i"] - got["lppd_i"]) <= 1e-12 * np.maximum(1.0, np.abs(got["lppd_i"])))


def test_ties_go_by_sample_index():
    """Equal ratios across the cut: the larger s is in the tail."""
    S = 40
    M, _ = LO.tail_count(S)
    assert M == 8
    ll = np.zeros((S, 1))
    ll[:20, 0] = -3.0        # 20 equal largest ratios, M = 8 of them in the tail
    ll[20:, 0] = -1.0
    lr, idx, cut = LO.select_tail(ll)
    assert idx[:, 0].tolist() == list(range(12, 20)) and cut[0] == 0.0 == lr[11, 0]


def test_smoothing_on_a_pareto_tail():
    """Ratios drawn from a Pareto law with k = 0.4: the fit recovers a k near it and the smoothed tail is ordered."""
    rng = np.random.default_rng(4)
    S = 4096
    ll = -(0.4 * rng.exponential(size=(S, 3)))   # lr = -ll: exp(lr) is Pareto with shape 0.4
    out, lw = LO.psis(ll)
    assert np.all(np.abs(out["khat_i"] - 0.4) < 0.2)
    _, idx, _ = LO.select_tail(ll)
    t = np.take_along_axis(lw, idx, axis=0)
    assert np.all(np.diff(t, axis=0) >= 0) and np.all(t <= 0)
    ex, _ = LO.psis(ll, exact=True)
    assert np.all(np.abs(np.float64(ex["khat_i"]) - out["khat_i"]) < 1e-9)


def test_stacking_closed_forms():
    rng = np.random.default_rng(5)
    e = rng.normal(-2, 1, 57)
    w, es, n, it = LO.stack(np.stack([e, e]))
    assert w.tobytes() == np.array([0.5, 0.5]).tobytes() and n == 57 and it == 1
    assert abs(es - e.sum()) < 1e-10
    w, es, n, it = LO.stack(np.stack([e + 50.0, e]))
    assert w[0] > 1 - 1e-12 and abs(w.sum() - 1) < 1e-12
    w, es, n, it = LO.stack(e[None, :])
    assert w.tolist() == [1.0] and it == 0 and abs(es - e.sum()) < 1e-10
    bad = np.stack([e, e])
    bad[0, ::2] = np.nan
    bad[1, 1::2] = -np.inf
    w, es, n, it = LO.stack(bad)
    assert n == 0 and np.all(np.isnan(w)) and np.isnan(es)
    bad = np.stack([e, e + 1])
    bad[0, :7] = np.nan
    assert LO.stack(bad)[2] == 50


def test_stacked_objective_never_decreases():
    rng = np.random.default_rng(6)
    e = rng.normal(-2, 1.5, (4, 90)) + np.array([0.0, 0.1, -0.3, 0.05])[:, None]
    w, es, n, it, objs = LO.stack(e, max_iter=200, trace=True)
    assert len(objs) == it + 1 and it > 3
    d = np.diff(np.array(objs))
    assert np.all(d >= -1e-12 * np.abs(objs[0]))
    assert objs[-1] > objs[0] and abs(w.sum() - 1) < 1e-12 and np.all(w >= 0)
    assert es >= np.max(e.sum(axis=1)) - 1e-9      # at least as good as the best single chain


def test_fit_stack_argument_checks():
    from transcriptioncycleinference_amd import mcmc

    for bad in (31, 4097, 64.5, True, -1):
        with pytest.raises(ValueError, match="stack"):
            mcmc.fit(None, thin=1, stack=bad)
    with pytest.raises(ValueError, match="thin"):
        mcmc.fit(None, thin=0, stack=64)
    assert mcmc.FitResult("x", [], [], [], np.zeros(0), 0, 0.0).MCMCstack is None
    assert "weights" in mcmc.STACK_FIELDS and "stacked_mean" in mcmc.STACK_FIELDS
