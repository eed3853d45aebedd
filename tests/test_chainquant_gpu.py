"""Posterior quantiles on the device (tci_chainquant.hip) against the numpy restatement of
tests/chainquant_oracle.py, bit for bit: the definition is exact (two true order statistics, two roundings in
a fixed order), so any difference is a bug.

The kernel has one path, a radix selection; its row loop has two constants, named here: a wavefront loads
CQ_RU rows together and the workgroup's four wavefronts advance CQ_STEP rows a step."""
import functools

import numpy as np
import pytest

import chaincov_oracle as CO
import chainquant_oracle as O
from test_chaincov_gpu import IDS, STAT_KEYS, _opts, _plan
from test_chaincov_gpu import same as same_cov

pytestmark = pytest.mark.gpu

CQ_RU = 8              # kCqRU
CQ_STEP = 4 * CQ_RU    # kCqWaves * kCqRU
PROBS5 = (0.0, 0.025, 0.5, 0.975, 1.0)
ROWS = sorted({1, 2, 3, 63, 64, 65, 255, 256, 257, CQ_RU - 1, CQ_RU, CQ_RU + 1, CQ_STEP - 1, CQ_STEP, CQ_STEP + 1})


@pytest.fixture(scope="module")
def lk(cells):
    from transcriptioncycleinference_amd import Likelihood

    with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as L:
        yield L


@functools.lru_cache(maxsize=None)
def case(rows, n_chains, ld, npar=None, seed=0):
    """A seeded random-walk chain with its s2 chain (computed once, never changed)."""
    chain = CO.walk_chain(100 * ld + rows + seed, rows, n_chains, ld, None if npar is None else list(npar))
    s2 = np.random.default_rng(rows + ld).gamma(3.0, 2.0, (rows, n_chains))
    chain.setflags(write=False)
    s2.setflags(write=False)
    return chain, s2


def check(lk, chain, s2, npar, probs, where=""):
    got = lk.chainquant(chain, s2, npar, probs)
    want = O.table(chain, s2, npar, probs)
    assert got.n_rows == chain.shape[0] and got.kernel_ms > 0, where
    assert got.q.shape == want["q"].shape and got.s2_q.shape == want["s2_q"].shape, where
    bad = np.argwhere(got.q.view(np.uint64) != want["q"].view(np.uint64))
    assert bad.size == 0, (where, "q differs at [chain, prob, column]", bad[:5].tolist())
    assert got.s2_q.tobytes() == want["s2_q"].tobytes(), (where, "s2_q")
    return got


@pytest.mark.parametrize("rows", ROWS)
def test_row_counts_around_every_tile_edge(lk, rows):
    chain, s2 = case(rows, 2, 10, (10, 7))
    got = check(lk, chain, s2, [10, 7], PROBS5, f"rows={rows}")
    assert np.all(np.isnan(got.q[1, :, 7:])) and np.all(np.isfinite(got.q[0])) and np.all(np.isfinite(got.q[1, :, :7]))
    assert got.q[0, 0].tobytes() == chain[:, 0].min(axis=0).tobytes()       # p = 0 and p = 1: the extremes
    assert got.q[0, 4].tobytes() == chain[:, 0].max(axis=0).tobytes()


def test_long_columns(lk):
    chain, s2 = case(20001, 2, 10)
    check(lk, chain, s2, None, PROBS5, "20001 rows")


@pytest.mark.parametrize("ld,npar", [(1, (1, 1, 0)), (10, (10, 3, 9)), (64, (64, 63, 1)), (65, (65, 64, 33)),
                                      (136, (136, 129, 64))])
def test_widths_and_chains_of_different_npar(lk, ld, npar):
    chain, s2 = case(65, 3, ld, npar)
    got = check(lk, chain, s2, list(npar), (0.025, 0.5, 0.975), f"ld={ld}")
    for c, P in enumerate(npar):                         # padding is NaN, the neighbours are untouched
        assert np.all(np.isnan(got.q[c, :, P:])) and np.all(np.isfinite(got.q[c, :, :P]))
    assert np.all(np.isfinite(got.s2_q))
    bare = check(lk, chain, None, list(npar), (0.025, 0.5, 0.975), f"ld={ld} without s2")
    assert np.all(np.isnan(bare.s2_q)) and bare.q.tobytes() == got.q.tobytes()
    if ld == 10:
        every = check(lk, chain, s2, None, (0.5,), "no npar")     # every column is real
        assert np.all(np.isfinite(every.q))
        one = lk.chainquant(chain[:, 1, :], s2[:, 1], probs=(0.5,))   # a 2-D chain is one chain
        assert one.q.shape == (1, 1, 10) and one.q[0].tobytes() == every.q[1].tobytes()


def test_probs(lk):
    chain, s2 = case(101, 2, 10, (10, 7))
    npar = [10, 7]
    check(lk, chain, s2, npar, (0.5,), "nq=1")
    check(lk, chain, s2, npar, np.linspace(0.0, 1.0, 16), "nq=16")
    check(lk, chain, s2, npar, np.random.default_rng(1).uniform(0, 1, 16), "nq=16, unsorted")
    got = check(lk, chain, s2, npar, (0.25, 1.0, 0.37, 0.25), "integer h, lo + 1 == n, a repeated prob")
    assert O.rank_of(101, 0.25) == (25, 0.0) and O.rank_of(101, 1.0) == (100, 0.0)
    y = np.sort(chain[:, 0, :], axis=0)
    assert got.q[0, 0].tobytes() == y[25].tobytes() and got.q[0, 1].tobytes() == y[100].tobytes()
    assert got.q[0, 3].tobytes() == got.q[0, 0].tobytes()
    dflt = lk.chainquant(chain, s2, npar)                 # the defaults
    assert dflt.probs.tolist() == [0.025, 0.5, 0.975] and O.same(dflt, O.table(chain, s2, npar))


def test_data_that_breaks_selections(lk):
    rows = 257
    rng = np.random.default_rng(17)
    cols = []
    cols.append(np.full(rows, 0.1))                                           # constant: one bucket in every pass
    cols.append(np.where(rng.random(rows) < 0.3, 2.5, -7.0))                  # two distinct values
    low = (np.full(rows, 1.5).view(np.uint64) | rng.integers(0, 256, rows).astype(np.uint64)).view(np.float64)
    cols.append(low)                                                          # only the last pass separates them
    mixed = rng.standard_normal(rows)
    mixed[[3, 77, 200]] = -0.0
    mixed[[4, 78, 201]] = 0.0
    cols.append(mixed)                                                        # both signs, -0.0 and +0.0
    zeros = np.where(rng.random(rows) < 0.5, -0.0, 0.0)
    cols.append(zeros)                                                        # nothing but the two zeros
    den = np.where(rng.random(rows) < 0.5, 5e-324 * rng.integers(1, 1000, rows), 1e300 * (1 + rng.random(rows)))
    cols.append(den)                                                          # denormals next to 1e300
    cols.append(-den)
    cols.append(np.sort(rng.standard_normal(rows)))                           # already sorted, and reversed
    cols.append(np.sort(rng.standard_normal(rows))[::-1])
    chain = np.ascontiguousarray(np.stack(cols, axis=1)[:, None, :])
    probs = (0.0, 0.01, 0.3, 0.5, 0.7, 0.99, 1.0)
    got = check(lk, chain, low, None, probs, "special columns")
    assert np.all(got.q[0, :, 0] == 0.1)
    assert got.q[0, 0, 1] == -7.0 and got.q[0, -1, 1] == 2.5
    # -0 sorts before +0: the largest of the two zeros is +0 (an interpolated zero is +0 either way: x - x = +0)
    assert got.q[0, -1, 4] == 0.0 and not np.signbit(got.q[0, -1, 4])


def test_chains_that_repeat_their_rows(lk):
    chain = O.repeated_rows(3, 1500, 3, 20)
    s2 = np.ascontiguousarray(O.repeated_rows(4, 1500, 3, 1)[:, :, 0])
    check(lk, chain, s2, [20, 13, 1], PROBS5, "repeated rows")


def test_the_golden_chain_rows(lk, chain):
    """Every fixture row as [step][cell][theta]: 299 chains of 10 rows and unequal length."""
    n = int(chain["cell_id"].max()) + 1
    steps = int(chain["step"].max()) + 1
    ld = max(len(r) for r in chain["rows"])
    x = np.full((steps, n, ld), 7.0)
    s2 = np.ones((steps, n))
    npar = np.zeros(n, np.int32)
    for r, c, s, v in zip(chain["rows"], chain["cell_id"], chain["step"], chain["s2"]):
        x[s, c, :len(r)] = r
        s2[s, c] = v
        npar[c] = len(r)
    check(lk, x, s2, npar, (0.025, 0.5, 0.975), "golden chain")


def test_non_finite_values_poison_exactly_their_column(lk):
    chain, s2 = (a.copy() for a in case(257, 2, 10))
    chain[0, 0, 2] = np.nan          # first row
    chain[128, 0, 5] = np.inf        # middle
    chain[256, 1, 3] = -np.inf       # last row
    s2[128, 1] = np.nan
    got = check(lk, chain, s2, None, PROBS5, "non-finite")
    nan = np.isnan(got.q)
    want = np.zeros_like(nan)
    want[0, :, 2] = want[0, :, 5] = want[1, :, 3] = True
    assert np.array_equal(nan, want)
    assert np.all(np.isnan(got.s2_q[1])) and np.all(np.isfinite(got.s2_q[0]))


def test_bits_do_not_depend_on_the_layout(lk):
    """An output's bits depend on the column's values, n and p alone."""
    npar = np.array([33, 16, 40], np.int32)
    chain, s2 = case(1001, 3, 40, (33, 16, 40))
    full = lk.chainquant(chain, s2, npar, PROBS5)
    assert O.same(full, O.table(chain, s2, npar, PROBS5))
    alone = lk.chainquant(chain[:, 1, :], s2[:, 1], npar[1:2], PROBS5)                  # evaluated alone
    assert alone.q[0].tobytes() == full.q[1].tobytes() and alone.s2_q[0].tobytes() == full.s2_q[1].tobytes()
    order = [2, 0, 1]                                                                   # at another position
    moved = lk.chainquant(np.ascontiguousarray(chain[:, order, :]), np.ascontiguousarray(s2[:, order]), npar[order],
                          PROBS5)
    assert moved.q.tobytes() == np.ascontiguousarray(full.q[order]).tobytes()
    assert moved.s2_q.tobytes() == np.ascontiguousarray(full.s2_q[order]).tobytes()
    wide = np.full((1001, 3, 70), 3.0)                                                  # a wider ld
    wide[:, :, :40] = chain
    w = lk.chainquant(wide, s2, npar, PROBS5)
    assert np.ascontiguousarray(w.q[:, :, :40]).tobytes() == full.q.tobytes() and np.all(np.isnan(w.q[:, :, 40:]))
    assert w.s2_q.tobytes() == full.s2_q.tobytes()


def test_bad_arguments_are_refused(lk):
    import ctypes as C

    from transcriptioncycleinference_amd import TciError, _lib

    x = np.zeros((30, 2, 4))
    for chain, kw, code in ((x[:0], {}, _lib.TCI_EINVAL),                                   # n_rows = 0
                            (x, dict(npar=[5, 1]), _lib.TCI_ERANGE),                        # npar > ld
                            (x, dict(npar=[-1, 1]), _lib.TCI_ERANGE)):
        with pytest.raises(TciError) as e:
            lk.chainquant(chain, **kw)
        assert e.value.code == code, kw
    for probs in ([], np.linspace(0, 1, 17), [-0.1], [np.nan]):                            # the binding's own checks
        with pytest.raises(ValueError):
            lk.chainquant(x, probs=probs)
    # ... and the library's, through the C ABI
    out = _lib.tci_chainquant_outputs()
    for nq, p0 in ((0, 0.5), (17, 0.5), (1, -0.1), (1, float("nan")), (2, 0.5)):
        o = _lib.tci_chainquant_options(nq)
        o.probs[0], o.probs[1] = p0, 1.5
        rc = lk._lib.tci_chainquant(lk._h, C.byref(o), _lib.ptr(x, _lib._dp), None, 30, 2, 4, None, C.byref(out))
        assert rc == _lib.TCI_EINVAL, (nq, p0)
    assert lk.chainquant(x[:1]).n_rows == 1            # and the context still works


# ---- tci_dram_run_reduced: the quantiles of the device chain ------------------------------------------

def same(a, b):
    return (a.q.tobytes() == b.q.tobytes() and a.s2_q.tobytes() == b.s2_q.tobytes() and a.n_rows == b.n_rows
            and a.probs.tobytes() == b.probs.tobytes())


@pytest.mark.parametrize("engine", ["fused", "batched", "walk"])
def test_dram_quantiles_equal_chainquant_of_the_returned_rows(lk, engine):
    from transcriptioncycleinference_amd.mcmc import dram_run

    npar = (7 + lk.cells.lengths[IDS]).astype(np.int32)
    res = dram_run(lk, *_plan(lk), _opts(engine=engine), quant=PROBS5)
    assert res.quant.n_rows == 301 and res.stats is None and res.cov is None      # rows 300 .. 600
    host = lk.chainquant(res.chain[299:], res.s2chain[299:], npar, PROBS5)
    assert same(res.quant, host)
    assert O.same(res.quant, O.table(res.chain[299:], res.s2chain[299:], npar, PROBS5))
    # without the host chain
    bare = dram_run(lk, *_plan(lk), _opts(engine=engine), quant=PROBS5, want_chain=False)
    assert bare.chain is None and bare.s2chain is None and same(bare.quant, host)
    # all three reductions at once: the statistics and matrices of tci_dram_run_cov
    three = dram_run(lk, *_plan(lk), _opts(engine=engine), quant=PROBS5, stats=True, cov=True, want_chain=False)
    two = dram_run(lk, *_plan(lk), _opts(engine=engine), stats=True, cov=True)
    assert same(three.quant, host) and two.quant is None and same_cov(three.cov, two.cov)
    for k in STAT_KEYS:
        assert getattr(three.stats, k).tobytes() == getattr(two.stats, k).tobytes(), k
    assert two.chain.tobytes() == res.chain.tobytes() and three.mean.tobytes() == res.mean.tobytes()


def test_dram_quantile_refusals(lk):
    from transcriptioncycleinference_amd import TciError, _lib
    from transcriptioncycleinference_amd.mcmc import DramOptions, dram_run

    for o in (DramOptions(n_steps=100, burnintime=50, stats_from=50, thin=0),               # thin == 0
              DramOptions(n_steps=100, burnintime=50, stats_from=101, thin=1)):             # no row in range
        with pytest.raises(TciError) as e:
            dram_run(lk, *_plan(lk), o, quant=(0.5,))
        assert e.value.code == _lib.TCI_EINVAL
    # one row in range is enough; thinned: kept rows 1, 8, 15, ..; the first at or past row 50 is row 50
    one = dram_run(lk, *_plan(lk), DramOptions(n_steps=100, burnintime=50, stats_from=100, thin=1), quant=(0.5,))
    assert one.quant.n_rows == 1
    for k, c in enumerate(IDS):
        P = 7 + int(lk.cells.lengths[c])
        assert one.quant.q[k, 0, :P].tobytes() == one.chain[99, k, :P].tobytes() and np.all(np.isnan(one.quant.q[k, 0, P:]))
    res = dram_run(lk, *_plan(lk), DramOptions(n_steps=300, burnintime=100, stats_from=50, thin=7, seed=2), quant=(0.1, 0.9))
    npar = (7 + lk.cells.lengths[IDS]).astype(np.int32)
    assert res.quant.n_rows == 43 - 7
    assert same(lk.chainquant(res.chain[7:], res.s2chain[7:], npar, (0.1, 0.9)), res.quant)


# ---- fit(..., quantiles=...) --------------------------------------------------------------------------

def test_fit_quantiles(lk):
    from transcriptioncycleinference_amd.mcmc import QUANT_FIELDS, THETA_INDEX, chain_theta, fit

    kw = dict(n_steps=600, n_burn=300, seed=4, thin=1)
    probs = (0.025, 0.25, 0.5, 0.975)
    fr = fit(lk, cells=IDS, quantiles=probs, **kw)
    assert [d["cell_index"] for d in fr.MCMCquant] == [c + 1 for c in IDS] and fr.MCMCdiag is None and fr.MCMCcov is None
    for d, ch, c in zip(fr.MCMCquant, fr.MCMCchain, IDS):
        N = int(lk.cells.lengths[c])
        assert tuple(d) == QUANT_FIELDS and d["q_dR"].shape == (4, N) and d["probs"].tolist() == list(probs)
        assert d["n_rows"] == 301 == len(ch["v_chain"])
        th = chain_theta(ch, N, np.arange(301))
        want = lk.chainquant(th, ch["s2chain"][299:], probs=probs)
        for name, col in THETA_INDEX.items():
            assert d["q_" + name].tobytes() == np.ascontiguousarray(want.q[0, :, col]).tobytes(), name
        assert d["q_dR"].tobytes() == np.ascontiguousarray(want.q[0, :, 7:]).tobytes()
        assert d["q_s2"].tobytes() == want.s2_q[0].tobytes()
        assert np.all(np.diff(d["q_v"]) >= 0) and np.all(np.isfinite(d["q_dR"]))
    plain = fit(lk, cells=IDS, **kw)                  # a fit without it has none, and the same chains
    assert plain.MCMCquant is None
    assert plain.MCMCchain[1]["dR_chain"].tobytes() == fr.MCMCchain[1]["dR_chain"].tobytes()
    shard = fit(lk, cells=IDS[1:2], quantiles=probs, **kw)   # a shard reproduces the full fit's bits
    assert shard.MCMCquant[0]["q_dR"].tobytes() == fr.MCMCquant[1]["q_dR"].tobytes()
