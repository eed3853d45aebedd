"""The multi-chain effective sample size on the device (tci_chainess.hip): against the longdouble restatement within
the derived bound (the windows equal) at the shapes where the kernels can go wrong, the special columns exactly, the
invariance of an output's bits to the layout, the run's own reduction against the chain it hands back for every
engine, fit(..., replicates=M, ess=True) and the refusals.

Shapes (chainess_oracle.NS): n = 1, 2, 3, 4, 5, 7, 8; 31 / 32 / 33 (the 32-row tile of k_ce_lags and of the moments);
63 .. 66 (the 64-lag tile for the whole chain, the 32-row tile for the halves); 127 .. 131 (the 64-lag tile for the
halves, two lag tiles); 255 / 256 / 257 (tci_chainrhat's 256-row segments, reused for the moments); 511 .. 514 (the same
for the halves); 1,100. ld = 1, 63, 64, 65, 130; M = 1, 2, 3, 4, 7; max_lag = 0, 1, 2, 3, 64, 65."""
import ctypes as C
import math

import numpy as np
import pytest

import chainess_oracle as O

pytestmark = pytest.mark.gpu

IDS = [3, 41, 120]       # three TestData cells
FIELDS = O.OUTPUTS + O.WINDOWS


@pytest.fixture(scope="module")
def lk(cells):
    from transcriptioncycleinference_amd import Likelihood

    with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
        yield lk


@pytest.fixture(scope="module")
def cases():
    return O.all_cases()


def same(a, b):
    return a.n_rows == b.n_rows and all(getattr(a, p + k).tobytes() == getattr(b, p + k).tobytes()
                                        for k in FIELDS for p in ("", "s2_"))


def test_every_shape_within_the_bound_and_the_windows_equal(lk, cases):
    worst_all = 0.0
    for c in cases:
        got = lk.chainess(c["chain"], c["s2"], c["npar"], c["group"], max_lag=c["max_lag"])
        assert got.n_rows == c["n"]
        worst = O.check(O.joined(got), c["ref"], c["n"], where=c["name"])
        print(f"{c['name']}: largest error / bound {max(worst.values()):.3f}")
        worst_all = max(worst_all, max(worst.values()))
        if c["s2"] is None:
            assert all(np.all(np.isnan(getattr(got, "s2_" + k))) for k in O.OUTPUTS)
            assert all(np.all(getattr(got, "s2_" + k) == -1) for k in O.WINDOWS)
    print(f"largest error as a fraction of the bound over all fixtures: {worst_all:.3f}")


def test_the_special_columns_exactly(lk, cases):
    sp = next(c for c in cases if c["name"] == "special")
    got = lk.chainess(sp["chain"], sp["s2"], sp["npar"], sp["group"])
    n, M = 300, 3
    cap = float(n * M) * math.log10(float(n * M))   # the split statistic's too: 2 M sequences of n / 2 rows
    # 1: the same constant everywhere (vplus = 0): NaN, the NaN stops the first pair examined
    assert np.isnan(got.tau[0, 1]) and np.isnan(got.ess[0, 1]) and np.isnan(got.mcse[0, 1]) and got.window[0, 1] == 2
    assert np.isnan(got.ess_split[0, 1]) and got.window_split[0, 1] == 2
    # 3: constant per chain, different (W = 0 < T): every rho is 1, every P 2, no pair stops: tau = -1 + 2 * 2 * (n / 2)
    assert got.tau[0, 3] == 2.0 * n - 1 and got.window[0, 3] == n and got.ess[0, 3] == n * M / (2.0 * n - 1)
    assert got.tau_split[0, 3] == 2.0 * (n // 2) - 1 and got.window_split[0, 3] == n // 2
    # 7: alternating +-1: mu = 0 and every product is exact; P_0 = 1 + rho(1) is tiny, tau < 0: ess is the cap
    assert got.tau[0, 7] < 0 and got.ess[0, 7] == cap and got.ess_split[0, 7] == cap
    assert got.mcse[0, 7] == lk.chainrhat(sp["chain"], sp["s2"]).pooled_std[0, 7] / np.sqrt(cap)
    # 4, 5, 8: NaN, +Inf, -Inf entries: NaN / -1
    for j in (4, 5, 8):
        assert all(np.isnan(getattr(got, k)[0, j]) for k in O.OUTPUTS) and got.window[0, j] == -1 == got.window_split[0, j]
    # 6: identical chains: T = 0, and one of them alone (m = 1) has the same exact tau: both are within the bound of it
    one = lk.chainess(sp["chain"][:, :1, 6:7])
    assert np.isfinite(got.tau[0, 6]) and got.window[0, 6] == one.window[0, 0]
    assert abs(got.tau[0, 6] - one.tau[0, 0]) <= 2 * O.bounds(sp["ref"], n)["tau"][0, 6]
    # padding and a group no chain carries
    pad = lk.chainess(sp["chain"], sp["s2"], np.full(3, 4, np.int32), np.array([2, 0, 2], np.int32))
    assert np.all(np.isnan(pad.ess[:, 4:])) and np.all(pad.window[:, 4:] == -1) and np.all(np.isnan(pad.tau[1]))
    assert np.all(pad.window[1] == -1) and pad.s2_window[1] == -1 and np.all(np.isfinite(pad.ess[2, :1]))
    # n < 4: split is NaN with window 0; n = 1: the classic one too
    tiny = lk.chainess(sp["chain"][:3, :, :1])
    assert np.isfinite(tiny.ess[0, 0]) and tiny.window[0, 0] == 2 and np.isnan(tiny.ess_split[0, 0])
    assert tiny.window_split[0, 0] == 0
    unit = lk.chainess(sp["chain"][:1, :, :1])
    assert np.isnan(unit.ess[0, 0]) and unit.window[0, 0] == 0 == unit.window_split[0, 0]


def test_a_cap_that_ends_an_unconverged_column(lk, cases):
    c = next(c for c in cases if c["name"] == "capped")
    got = lk.chainess(c["chain"], c["s2"], c["npar"], c["group"], max_lag=c["max_lag"])
    assert np.all(np.isposinf(got.tau[0])) and np.all(got.ess[0] == 0.0) and np.all(got.window[0] == 10)
    assert np.all(np.isposinf(got.mcse[0]))
    free = lk.chainess(c["chain"], c["s2"], c["npar"], c["group"])
    assert np.all(np.isfinite(free.tau[0])) and np.all(free.window[0] > 10)


def test_bits_do_not_depend_on_the_layout(lk):
    """An output's bits depend on the group's columns in chain order, on n and on max_lag alone."""
    n, M, ld = 257, 3, 37
    npar = np.full(M, 33, np.int32)
    chain, s2 = O.ar1_chains(9, n, M, ld, npar)
    for max_lag in (0, 65):
        alone = lk.chainess(chain, s2, npar, max_lag=max_lag)
        others, s2o = O.ar1_chains(10, n, 40, 70, np.full(40, 70))
        pos = [4, 19, 42]
        big = np.zeros((n, 43, 70))
        big_s2 = np.zeros((n, 43))
        rest = [c for c in range(43) if c not in pos]
        big[:, rest], big_s2[:, rest] = others, s2o
        big[:, pos, :ld], big_s2[:, pos] = chain, s2
        big[:, pos, 33:] = 3.0                                   # padding of the group's chains: masked by npar
        bnpar = np.full(43, 70, np.int32)
        bnpar[pos] = 33
        # the others in groups after it, in groups before it in another order, and in no group at all
        for mine, ids in ((0, lambda k: 1 + k % 4), (4, lambda k: (7 * k) % 4), (0, lambda k: -1)):
            group = np.zeros(43, np.int32)
            group[rest] = [ids(k) for k in range(40)]
            group[pos] = mine
            got = lk.chainess(big, big_s2, bnpar, group, max_lag=max_lag)
            for k in FIELDS:
                assert getattr(got, k)[mine, :ld].tobytes() == getattr(alone, k)[0].tobytes(), (mine, k)
                assert getattr(got, "s2_" + k)[mine] == getattr(alone, "s2_" + k)[0], (mine, k)
            assert np.all(np.isnan(got.ess[mine, 33:])) and np.all(got.window[mine, 33:] == -1)


def test_bad_arguments_are_refused(lk):
    from transcriptioncycleinference_amd import _lib

    x = np.zeros((20, 3, 2))
    out = _lib.tci_chainess_outputs()
    P, I = (lambda a: _lib.ptr(a, _lib._dp)), (lambda a: _lib.ptr(np.ascontiguousarray(a, np.int32), _lib._i32p))  # noqa: E731

    def call(opt=None, rows=20, npar=None, group=None, ng=1, chain=x, o=out):
        rc = lk._lib.tci_chainess(lk._h, None if opt is None else C.byref(opt), P(chain), None, rows, 3, 2,
                                  None if npar is None else I(npar), None if group is None else I(group), ng,
                                  None if o is None else C.byref(o))
        return rc, lk._lib.tci_last_error(lk._h).decode()

    assert call()[0] == _lib.TCI_OK
    d = _lib.tci_chainess_options(5, 5)
    assert lk._lib.tci_chainess_defaults(C.byref(d)) == _lib.TCI_OK and (d.max_lag, d.flags) == (0, 0)
    rc, msg = call(opt=_lib.tci_chainess_options(0, 1))
    assert rc == _lib.TCI_EINVAL and "flags" in msg
    rc, msg = call(opt=_lib.tci_chainess_options(-1, 0))
    assert rc == _lib.TCI_EINVAL and "max_lag" in msg
    rc, msg = call(npar=[2, 1, 2], group=[1, 0, 0], ng=2)
    assert rc == _lib.TCI_EINVAL and "group 0" in msg and "npar" in msg
    assert call(npar=[2, 1, 2], group=[0, 1, 0], ng=2)[0] == _lib.TCI_OK
    assert call(group=[0, 2, 0], ng=2)[0] == _lib.TCI_ERANGE
    assert call(group=[0, -2, 0], ng=2)[0] == _lib.TCI_ERANGE
    assert call(npar=[2, 3, 2])[0] == _lib.TCI_ERANGE
    for kw in (dict(rows=0), dict(ng=0), dict(ng=4), dict(chain=None), dict(o=None)):
        assert call(**kw)[0] == _lib.TCI_EINVAL, kw


def _opts(**kw):
    from transcriptioncycleinference_amd.mcmc import DramOptions

    return DramOptions(**{**dict(n_steps=600, burnintime=200, stats_from=200, thin=1, seed=7), **kw})


def _plan(lk, replicates=1):
    from transcriptioncycleinference_amd.mcmc import plan_fit

    p = plan_fit(lk.cells, IDS, 11, replicates=replicates)
    return (np.tile(np.array(IDS, np.int32), replicates), p.x0, p.lower, p.upper, p.prior_mu, p.prior_sig, p.qcov_diag,
            1.0)


def test_the_run_reduction_is_chainess_of_the_chain_handed_back(lk):
    """tci_dram_run_ess's own reduction against chainess of the rows it returns, for every engine, on 3 cells x 3
    replicates; R-hat beside it is what tci_dram_run_rhat gives; the refusals."""
    from transcriptioncycleinference_amd import TciError, _lib
    from transcriptioncycleinference_amd.mcmc import dram_run, replicate_keys

    plan = _plan(lk, 3)
    group = np.tile(np.arange(3, dtype=np.int32), 3)
    keys = replicate_keys(IDS, 3)
    npar = (7 + lk.cells.lengths[np.tile(IDS, 3)]).astype(np.int32)
    first = None
    for engine in ("auto", "fused", "batched", "walk"):
        res = dram_run(lk, *plan, _opts(engine=engine), chain_keys=keys, group=group, ess=True, max_lag=100)
        assert res.ess.n_rows == 401 and res.ess.max_lag == 100
        host = lk.chainess(res.chain[199:], res.s2chain[199:], npar, group, max_lag=100)
        assert same(res.ess, host), engine
        first = first or res
        assert same(res.ess, first.ess), engine
    P = 7 + int(lk.cells.lengths[3])
    assert np.all(first.ess.ess[0, :P] >= 0) and np.all(first.ess.window[0, :P] >= 2)
    plain = dram_run(lk, *plan, _opts(), chain_keys=keys, group=group, want_chain=False)
    bare = dram_run(lk, *plan, _opts(), chain_keys=keys, group=group, ess=True, max_lag=100, want_chain=False)
    assert plain.ess is None and bare.chain is None and same(bare.ess, first.ess)
    for k in ("rhat", "rhat_split", "pooled_mean", "pooled_std", "s2_rhat", "s2_pooled_std"):
        assert getattr(bare.rhat, k).tobytes() == getattr(plain.rhat, k).tobytes(), k
    for o in (_opts(thin=0), _opts(stats_from=600)):          # no kept rows; one row in range
        with pytest.raises(TciError) as e:
            dram_run(lk, *plan, o, group=group, chain_keys=keys, ess=True)
        assert e.value.code == _lib.TCI_EINVAL and "tci_dram_run_ess" in str(e.value)
    with pytest.raises(TciError) as e:                        # cell 120 is shorter than cells 3 and 41: mixed npar
        dram_run(lk, *plan, _opts(), group=np.zeros(9, np.int32), chain_keys=keys, ess=True)
    assert e.value.code == _lib.TCI_EINVAL and "group 0" in str(e.value)
    with pytest.raises(ValueError):
        dram_run(lk, *plan, _opts(), chain_keys=keys, ess=True)


def test_fit_replicates_with_ess(lk):
    from transcriptioncycleinference_amd.mcmc import ESS_FIELDS, fit

    kw = dict(n_steps=600, n_burn=200, thin=1, seed=11, cells=IDS, replicates=3)
    base = fit(lk, **kw)
    with_ess = fit(lk, ess=True, max_lag=50, **kw)
    assert base.MCMCess is None and len(with_ess.MCMCess) == 3

    def flat(x):
        if isinstance(x, dict):
            return b"".join(flat(x[k]) for k in sorted(x))
        return np.ascontiguousarray(x).tobytes()

    for name in ("MCMCresults", "MCMCchain", "MCMCplot", "MCMCrhat"):   # the same fit without ess, byte for byte
        for a, b in zip(getattr(base, name), getattr(with_ess, name)):
            assert flat(a) == flat(b), name
    assert with_ess.accept_rate.tobytes() == base.accept_rate.tobytes()
    assert with_ess.final_theta.tobytes() == base.final_theta.tobytes()
    for k, c in enumerate(IDS):
        e, P = with_ess.MCMCess[k], 7 + int(lk.cells.lengths[c])
        assert tuple(e) == ESS_FIELDS and e["n_rows"] == 401 and e["n_chains"] == 3 and e["cell_index"] == c + 1
        assert e["max_lag"] == 50 and all(e[f].shape == (P + 1,) for f in O.OUTPUTS + O.WINDOWS)
        assert e["window"].dtype == np.int32 and np.all(e["window"] >= 2) and np.all(e["window"] <= 50)
        assert not np.any(np.isnan(e["ess"])) and e["ess_min"] == min(e["ess"].min(), e["ess_split"].min())
    with pytest.raises(ValueError):
        fit(lk, ess=True, **{**kw, "replicates": 1})
