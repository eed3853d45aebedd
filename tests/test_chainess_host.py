"""The restatement of tci_chainess (chainess_oracle) on the CPU: its FP64 form meets the derived bound against its
longdouble twin in three summation orders, the estimate is right on AR(1) chains, the stated consequences of the
definition hold, the bound is tight enough to catch a wrong kernel, and the bindings check their arguments."""
import numpy as np
import pytest

import chainess_oracle as O


@pytest.fixture(scope="module")
def cases():
    return O.all_cases()


def test_fp64_meets_the_bound_in_every_order(cases):
    for c in cases:
        for order in O.ORDERS:
            got = O.table(c["chain"], c["s2"], c["npar"], c["group"], c["max_lag"], order=order)
            O.check(got, c["ref"], c["n"], where=(c["name"], order))


def test_every_fixture_keeps_its_pairs_away_from_the_stop(cases):
    assert all(O.margins_hold(c["ref"], c["n"]) for c in cases)


@pytest.mark.parametrize("phi", [0.0, 0.5, 0.9])
def test_ar1_ess_is_the_textbook_value(phi):
    n, M = 1000, 4
    chain, _ = O.ar1_chains(5, n, M, 1, [1] * M, phi=phi, shift=0.0)
    ess = float(O.table(chain)["ess"][0, 0])
    want = M * n * (1 - phi) / (1 + phi)
    print(f"phi {phi}: ess {ess:.0f} against {want:.0f}")
    assert abs(ess - want) <= 0.25 * want


def test_a_shifted_chain_leaves_almost_no_sample():
    n, M = 1000, 4
    chain, _ = O.ar1_chains(6, n, M, 1, [1] * M, phi=0.3, shift=0.0)
    chain[:, 0, 0] += 30.0 * chain[:, 1:, 0].std()
    t = O.table(chain)
    print(f"ess {float(t['ess'][0, 0]):.2f}, window {int(t['window'][0, 0])}")
    assert t["window"][0, 0] == 2 * (n // 2) and t["ess"][0, 0] < 2 * M


def test_the_stated_consequences():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((40, 3, 1))
    for n in (1, 2, 3):                                       # L < 2: NaN; n = 2, 3: P_0 only
        t = O.table(x[:n])
        assert np.isnan(t["ess_split"][0, 0]) and t["window_split"][0, 0] == 0
        assert (np.isnan(t["ess"][0, 0]) and t["window"][0, 0] == 0) if n == 1 else t["window"][0, 0] == 2
    assert np.isfinite(O.table(x[:4])["ess_split"][0, 0])
    t = O.table(x[:, :1])                                     # m = 1: the single-chain estimate
    assert np.isfinite(t["ess"][0, 0]) and np.isfinite(t["mcse"][0, 0])
    walk = np.cumsum(x, axis=0)                               # the cap ends it: +Inf / 0, window 2 s
    t = O.table(walk, max_lag=5)
    assert np.isposinf(t["tau"][0, 0]) and t["ess"][0, 0] == 0 and t["window"][0, 0] == 6
    t = O.table(walk, max_lag=39)                             # running out of lags at L - 1 is finite
    assert np.isfinite(t["tau"][0, 0])
    const = np.full((40, 3, 1), 2.5)                          # vplus == 0: NaN
    t = O.table(const)
    assert np.isnan(t["tau"][0, 0]) and np.isnan(t["ess"][0, 0]) and np.isnan(t["mcse"][0, 0])
    steps = const * np.array([1.0, 2.0, 3.0])[None, :, None]  # W = 0 < T: every rho is 1
    t = O.table(steps)
    assert t["tau"][0, 0] == 2 * 40 - 1 and t["window"][0, 0] == 40
    for v in (np.nan, np.inf, -np.inf):                       # a non-finite entry: NaN / -1
        y = x.copy()
        y[7, 2, 0] = v
        t = O.table(y)
        assert all(np.isnan(t[k][0, 0]) for k in O.OUTPUTS) and t["window"][0, 0] == -1 == t["window_split"][0, 0]
    t = O.table(x, npar=[0, 0, 0], group=[2, 0, 2])           # padding and a group id no chain carries
    assert np.all(np.isnan(t["ess"])) and np.all(t["window"][:, 0] == -1) and t["ess"].shape == (3, 2)
    with pytest.raises(AssertionError):
        O.table(np.zeros((9, 2, 3)), npar=[3, 2])             # mixed npar within a group


def test_the_bound_on_ess_is_below_1e8_of_ess(cases):
    worst = 0.0
    for c in cases:
        b = O.bounds(c["ref"], c["n"])
        for k in ("ess", "ess_split"):
            e = np.asarray(c["ref"][k], np.float64)
            ok = np.isfinite(e) & (e > 0)
            if ok.any():
                worst = max(worst, float(np.max(b[k][ok] / e[ok])))
                assert np.all(b[k][ok] < 1e-8 * e[ok]), (c["name"], k)
    print(f"largest derived bound on ess / ess: {worst:.2e}")


def test_arguments_are_checked_without_a_gpu():
    from transcriptioncycleinference_amd import mcmc
    from transcriptioncycleinference_amd.likelihood import ChainEss, rhat_groups

    with pytest.raises(ValueError):
        ChainEss.empty(2, 3, max_lag=-1)
    with pytest.raises(ValueError):
        ChainEss.empty(2, 3, max_lag=1.5)
    e = ChainEss.empty(2, 3, max_lag=7)
    assert e.ess.shape == (2, 3) and e.window.dtype == np.int32 and np.all(e.s2_window == -1) and e.options().max_lag == 7
    with pytest.raises(ValueError):
        rhat_groups([0, 0], 2, npar=[3, 2])
    assert "MCMCess" in mcmc.FitResult.__dataclass_fields__ and mcmc.ESS_FIELDS[:2] == ("ess", "ess_split")
    with pytest.raises(ValueError):                           # ess needs group (checked before the library is touched)
        mcmc.dram_run(None, np.zeros(1, np.int32), *(np.ones((1, 8)),) * 6, 1.0, mcmc.DramOptions(), ess=True)
