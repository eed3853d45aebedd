"""Marginal densities and histograms on the device (tci_chaindens.hip) against the numpy restatement of
tests/chaindens_oracle.py: range, the grid and counts bit for bit (pinned IEEE operations on exact order
statistics), bw and dens within the bounds derived in the oracle's docstring.

The kernels cut the rows into segments of CD_SEG rows (one workgroup each, the block the density kernel stages in
LDS); in the moments passes a wavefront loads CD_RU rows together and the four wavefronts advance CD_STEP rows a
step; a wavefront evaluates CD_KU grid points together."""
import functools

import numpy as np
import pytest

import chaincov_oracle as CO
import chaindens_oracle as O
import chainquant_oracle as QO
from test_chaincov_gpu import IDS, STAT_KEYS, _opts, _plan
from test_chaincov_gpu import same as same_cov

pytestmark = pytest.mark.gpu

CD_RU = 8              # kCdRU
CD_STEP = 4 * CD_RU    # kCdWaves * kCdRU
CD_SEG = 256           # kCdSeg
CD_KU = 4              # kCdKU
ROWS = sorted({2, 3, 63, 64, 65, 255, 256, 257, CD_RU - 1, CD_RU, CD_RU + 1, CD_STEP - 1, CD_STEP, CD_STEP + 1,
               CD_SEG - 1, CD_SEG, CD_SEG + 1, 2 * CD_SEG - 1, 2 * CD_SEG, 2 * CD_SEG + 1})
KEYS = ("range", "bw", "dens", "counts", "s2_range", "s2_bw", "s2_dens", "s2_counts")


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


def check(lk, chain, s2, npar, where="", **opt):
    got = lk.chaindens(chain, s2, npar, **opt)
    want = O.table(chain, s2, npar, **opt)
    assert got.n_rows == chain.shape[0] and got.kernel_ms > 0, where
    worst = O.compare(got, want, chain.shape[0], where)
    print(f"chaindens {where}: bw and dens errors / bound {worst}")
    return got


def same(a, b):
    return all(getattr(a, k).tobytes() == getattr(b, k).tobytes() for k in KEYS) and a.n_rows == b.n_rows


@pytest.mark.parametrize("rows", ROWS)
def test_row_counts_around_every_block_and_segment_edge(lk, rows):
    chain, s2 = case(rows, 2, 10, (10, 7))
    got = check(lk, chain, s2, [10, 7], f"rows={rows}")
    assert np.all(np.isnan(got.dens[1, :, 7:])) and np.all(got.counts[1, :, 7:] == -1)
    assert np.all(got.counts[0].sum(axis=0) == rows) and np.all(got.s2_counts.sum(axis=1) == rows)
    assert got.range[0, 0].tobytes() == chain[:, 0].min(axis=0).tobytes()
    assert got.range[0, 1].tobytes() == chain[:, 0].max(axis=0).tobytes()
    assert np.all(got.counts[0, -1] >= 1) and np.all(got.counts[0, 0] >= 1)      # xmax in the last bin, xmin in bin 0


def test_long_columns_run_many_segments(lk):
    chain, s2 = case(20001, 2, 10)
    check(lk, chain, s2, None, "20001 rows")


@pytest.mark.parametrize("ld,npar", [(1, (1, 1, 0)), (10, (10, 3, 9)), (64, (64, 63, 1)), (65, (65, 64, 33)),
                                      (136, (136, 129, 64))])
def test_widths_and_chains_of_different_npar(lk, ld, npar):
    chain, s2 = case(65, 3, ld, npar)
    got = check(lk, chain, s2, list(npar), f"ld={ld}")
    for c, P in enumerate(npar):                         # padding is NaN / -1, the neighbours are untouched
        assert np.all(np.isnan(got.dens[c, :, P:])) and np.all(np.isfinite(got.dens[c, :, :P]))
        assert np.all(got.counts[c, :, P:] == -1) and np.all(got.counts[c, :, :P] >= 0)
        assert np.all(np.isnan(got.bw[c, P:])) and np.all(np.isnan(got.range[c, :, P:]))
    assert np.all(np.isfinite(got.s2_dens)) and np.all(got.s2_counts >= 0)
    bare = check(lk, chain, None, list(npar), f"ld={ld} without s2")
    assert np.all(np.isnan(bare.s2_dens)) and np.all(bare.s2_counts == -1) and np.all(np.isnan(bare.s2_bw))
    assert all(getattr(bare, k).tobytes() == getattr(got, k).tobytes() for k in KEYS[:4])
    if ld == 10:
        every = check(lk, chain, s2, None, "no npar")     # every column is real
        assert np.all(np.isfinite(every.dens))
        one = lk.chaindens(chain[:, 1, :], s2[:, 1])      # a 2-D chain is one chain
        assert one.dens.shape == (1, 100, 10) and one.dens[0].tobytes() == every.dens[1].tobytes()


@pytest.mark.parametrize("B", [1, 2, 20, 256])
@pytest.mark.parametrize("G", [2, 3, 100, 255, 256, CD_KU * 4 - 1, CD_KU * 4, CD_KU * 4 + 1])
def test_grid_and_bin_counts(lk, G, B):
    chain, s2 = case(101, 2, 10, (10, 7))
    got = check(lk, chain, s2, [10, 7], f"G={G} B={B}", n_grid=G, n_bins=B)
    assert got.dens.shape == (2, G, 10) and got.counts.shape == (2, B, 10) and (got.n_grid, got.n_bins) == (G, B)


def test_bandwidth_scale_and_defaults(lk):
    chain, s2 = case(257, 2, 10, (10, 7))
    one = check(lk, chain, s2, [10, 7], "bw_scale=1")
    assert (one.n_grid, one.n_bins, one.bw_scale) == (100, 20, 1.0)
    for s in (0.37, 2.5):
        got = check(lk, chain, s2, [10, 7], f"bw_scale={s}", bw_scale=s)
        assert got.range.tobytes() == one.range.tobytes() and got.counts.tobytes() == one.counts.tobytes()
        assert np.allclose(got.bw[0], s * one.bw[0], rtol=1e-14, atol=0)


def test_special_columns(lk):
    rows = 257
    rng = np.random.default_rng(17)
    cols = []
    cols.append(np.full(rows, 0.1))                                           # constant: bw 0, dens NaN, bin 0
    cols.append(np.where(np.arange(rows) % 10 == 3, -7.0, 2.5))               # two values, iqr == 0: bw from sd
    cols.append(np.where(rng.random(rows) < 0.5, 2.5, -7.0))                  # two values, iqr > 0
    mixed = rng.standard_normal(rows)
    mixed[[3, 77, 200]] = -0.0
    mixed[[4, 78, 201]] = 0.0
    cols.append(mixed)                                                        # both signs, -0.0 and +0.0
    cols.append(np.where(rng.random(rows) < 0.5, -0.0, 0.0))                  # nothing but the two zeros: r == 0
    cols.append(np.abs(rng.standard_normal(rows)) + 0.5)
    cols[-1][5] = -0.0                                                        # the minimum is -0
    cols.append(5.0 + 1e-6 * rng.standard_normal(rows))                       # near-constant: the hierarchical v
    top = rng.random(rows)
    top[[0, 100, 256]] = 1.0
    top[[1, 101]] = 0.0
    cols.append(top)                                                          # xmax repeated: each in the last bin
    cols.append(np.sort(rng.standard_normal(rows)))                           # already sorted, and reversed
    cols.append(np.sort(rng.standard_normal(rows))[::-1])
    cols.append(np.arange(rows, dtype=np.float64))                            # values on the bin edges (B = 16: r / B = 16)
    chain = np.ascontiguousarray(np.stack(cols, axis=1)[:, None, :])
    got = check(lk, chain, cols[6], None, "special columns", n_bins=16)
    assert got.bw[0, 0] == 0.0 and np.all(np.isnan(got.dens[0, :, 0])) and got.counts[0, :, 0].tolist() == [rows] + [0] * 15
    assert got.range[0, :, 0].tolist() == [0.1, 0.1]
    assert got.bw[0, 1] > 0 and QO.quantiles(cols[1], [0.25, 0.75]).tolist() == [2.5, 2.5]
    assert got.counts[0, 0, 1] + got.counts[0, -1, 1] == rows and got.counts[0, 0, 1] == 26
    assert np.signbit(got.range[0, 0, 4]) and not np.signbit(got.range[0, 1, 4]) and got.range[0, 1, 4] == 0.0
    assert got.bw[0, 4] == 0.0 and got.counts[0, 0, 4] == rows
    assert np.signbit(got.range[0, 0, 5]) and got.range[0, 0, 5] == 0.0
    # range [0, 1], 16 bins: x * 16 is exact, so the last bin holds the rows >= 15/16, the three at xmax included
    assert got.counts[0, -1, 7] == np.sum(top >= 15 / 16) >= 3 and got.counts[0, 0, 7] == np.sum(top < 1 / 16) >= 2
    assert got.counts[0, :, 10].tolist() == [16] * 15 + [17]


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
    check(lk, x, s2, npar, "golden chain", n_grid=16)


def test_non_finite_values_poison_exactly_their_column(lk):
    chain, s2 = (a.copy() for a in case(513, 2, 10))
    chain[0, 0, 2] = np.nan          # first row
    chain[300, 0, 5] = np.inf        # in the second segment
    chain[512, 1, 3] = -np.inf       # last row
    s2[128, 1] = np.nan
    got = check(lk, chain, s2, None, "non-finite")
    want = np.zeros((2, 10), bool)
    want[0, 2] = want[0, 5] = want[1, 3] = True
    assert np.array_equal(np.isnan(got.bw), want) and np.array_equal(np.all(np.isnan(got.dens), axis=1), want)
    assert np.array_equal(np.all(got.counts == -1, axis=1), want) and np.array_equal(np.any(got.counts == -1, axis=1), want)
    assert np.array_equal(np.all(np.isnan(got.range), axis=1), want)
    assert np.all(np.isnan(got.s2_dens[1])) and np.all(got.s2_counts[1] == -1) and np.all(np.isfinite(got.s2_dens[0]))


def test_bits_do_not_depend_on_the_layout(lk):
    """An output's bits depend on the column's values, n and the options alone."""
    npar = np.array([33, 16, 40], np.int32)
    chain, s2 = case(1001, 3, 40, (33, 16, 40))
    full = check(lk, chain, s2, npar, "layout")
    alone = lk.chaindens(chain[:, 1, :], s2[:, 1], npar[1:2])                           # evaluated alone
    for k in KEYS:
        assert getattr(alone, k)[0].tobytes() == getattr(full, k)[1].tobytes(), k
    order = [2, 0, 1]                                                                   # at another position
    moved = lk.chaindens(np.ascontiguousarray(chain[:, order, :]), np.ascontiguousarray(s2[:, order]), npar[order])
    for k in KEYS:
        assert getattr(moved, k).tobytes() == np.ascontiguousarray(getattr(full, k)[order]).tobytes(), k
    wide = np.full((1001, 3, 70), 3.0)                                                  # a wider ld
    wide[:, :, :40] = chain
    w = lk.chaindens(wide, s2, npar)
    for k in KEYS[:4]:
        assert np.ascontiguousarray(getattr(w, k)[..., :40]).tobytes() == getattr(full, k).tobytes(), k
    assert np.all(np.isnan(w.dens[..., 40:])) and np.all(w.counts[..., 40:] == -1)
    for k in KEYS[4:]:
        assert getattr(w, k).tobytes() == getattr(full, k).tobytes(), k


def test_bad_arguments_are_refused(lk):
    import ctypes as C

    from transcriptioncycleinference_amd import TciError, _lib

    x = np.random.default_rng(2).standard_normal((30, 2, 4))
    for chain, kw, code in ((x[:1], {}, _lib.TCI_EINVAL),                                   # n_rows = 1
                            (x[:0], {}, _lib.TCI_EINVAL),
                            (x, dict(npar=[5, 1]), _lib.TCI_ERANGE),                        # npar > ld
                            (x, dict(npar=[-1, 1]), _lib.TCI_ERANGE)):
        with pytest.raises(TciError) as e:
            lk.chaindens(chain, **kw)
        assert e.value.code == code, kw
    for kw in (dict(n_grid=1), dict(n_grid=257), dict(n_bins=0), dict(n_bins=257), dict(bw_scale=0.0),
               dict(bw_scale=float("nan")), dict(bw_scale=float("inf"))):                   # the binding's own checks
        with pytest.raises(ValueError):
            lk.chaindens(x, **kw)
    # ... and the library's, through the C ABI
    out = _lib.tci_chaindens_outputs()
    for G, B, s in ((1, 20, 1.0), (257, 20, 1.0), (100, 0, 1.0), (100, 257, 1.0), (100, 20, 0.0), (100, 20, -1.0),
                    (100, 20, float("nan")), (100, 20, float("inf"))):
        o = _lib.tci_chaindens_options(G, B, s)
        rc = lk._lib.tci_chaindens(lk._h, C.byref(o), _lib.ptr(x, _lib._dp), None, 30, 2, 4, None, C.byref(out))
        assert rc == _lib.TCI_EINVAL, (G, B, s)
    rc = lk._lib.tci_chaindens(lk._h, None, _lib.ptr(x, _lib._dp), None, 30, 2, 4, None, None)   # null outputs
    assert rc == _lib.TCI_EINVAL
    assert lk.chaindens(x[:2]).n_rows == 2             # and the context still works


# ---- tci_dram_run_reduced: the densities of the device chain ------------------------------------------

@pytest.mark.parametrize("engine", ["fused", "batched", "walk"])
def test_dram_densities_equal_chaindens_of_the_returned_rows(lk, engine):
    from test_chainquant_gpu import same as same_quant
    from transcriptioncycleinference_amd.mcmc import dram_run

    npar = (7 + lk.cells.lengths[IDS]).astype(np.int32)
    res = dram_run(lk, *_plan(lk), _opts(engine=engine), dens=True)
    assert res.dens.n_rows == 301 and res.stats is None and res.cov is None and res.quant is None   # rows 300 .. 600
    host = lk.chaindens(res.chain[299:], res.s2chain[299:], npar)
    assert same(res.dens, host)
    O.compare(res.dens, O.table(res.chain[299:], res.s2chain[299:], npar), 301, engine)
    # without the host chain, and with options
    bare = dram_run(lk, *_plan(lk), _opts(engine=engine), dens=True, want_chain=False)
    assert bare.chain is None and bare.s2chain is None and same(bare.dens, host)
    opt = dict(n_grid=33, n_bins=7, bw_scale=0.5)
    other = dram_run(lk, *_plan(lk), _opts(engine=engine), dens=opt, want_chain=False)
    assert same(other.dens, lk.chaindens(res.chain[299:], res.s2chain[299:], npar, **opt))
    # all four reductions at once: the others are what they are without the densities
    probs = (0.025, 0.5, 0.975)
    four = dram_run(lk, *_plan(lk), _opts(engine=engine), dens=True, quant=probs, stats=True, cov=True, want_chain=False)
    three = dram_run(lk, *_plan(lk), _opts(engine=engine), quant=probs, stats=True, cov=True)
    assert same(four.dens, host) and three.dens is None
    assert same_quant(four.quant, three.quant) and same_cov(four.cov, three.cov)
    for k in STAT_KEYS:
        assert getattr(four.stats, k).tobytes() == getattr(three.stats, k).tobytes(), k
    assert three.chain.tobytes() == res.chain.tobytes() and four.mean.tobytes() == res.mean.tobytes()


def test_dram_density_refusals(lk):
    from transcriptioncycleinference_amd import TciError, _lib
    from transcriptioncycleinference_amd.mcmc import DramOptions, dram_run

    for o in (DramOptions(n_steps=100, burnintime=50, stats_from=50, thin=0),               # thin == 0
              DramOptions(n_steps=100, burnintime=50, stats_from=101, thin=1),              # no row in range
              DramOptions(n_steps=100, burnintime=50, stats_from=100, thin=1)):             # one row in range
        with pytest.raises(TciError) as e:
            dram_run(lk, *_plan(lk), o, dens=True)
        assert e.value.code == _lib.TCI_EINVAL
    for bad in (dict(n_grid=1), dict(n_bins=1000), dict(bw_scale=-2.0)):
        with pytest.raises(ValueError):
            dram_run(lk, *_plan(lk), DramOptions(n_steps=100, burnintime=50, stats_from=50, thin=1), dens=bad)
    # two rows in range are enough, and the context still works after the refusals
    two = dram_run(lk, *_plan(lk), DramOptions(n_steps=100, burnintime=50, stats_from=99, thin=1), dens=True)
    assert two.dens.n_rows == 2
    npar = (7 + lk.cells.lengths[IDS]).astype(np.int32)
    assert same(two.dens, lk.chaindens(two.chain[98:], two.s2chain[98:], npar))
    res = dram_run(lk, *_plan(lk), DramOptions(n_steps=300, burnintime=100, stats_from=50, thin=7, seed=2), dens=True)
    assert res.dens.n_rows == 43 - 7                  # kept rows 1, 8, 15, ..; the first at or past row 50 is row 50
    assert same(lk.chaindens(res.chain[7:], res.s2chain[7:], npar), res.dens)


# ---- fit(..., density=...) ----------------------------------------------------------------------------

def test_fit_density(lk):
    from transcriptioncycleinference_amd.mcmc import DENS_FIELDS, chain_theta, fit

    kw = dict(n_steps=600, n_burn=300, seed=4, thin=1)
    opt = dict(n_grid=50, n_bins=10)
    fr = fit(lk, cells=IDS, density=opt, **kw)
    assert [d["cell_index"] for d in fr.MCMCdens] == [c + 1 for c in IDS]
    assert fr.MCMCdiag is None and fr.MCMCcov is None and fr.MCMCquant is None
    for d, ch, c in zip(fr.MCMCdens, fr.MCMCchain, IDS):
        N = int(lk.cells.lengths[c])
        P = 7 + N
        assert tuple(d) == DENS_FIELDS and d["n_rows"] == 301 == len(ch["v_chain"])
        assert d["grid"].shape == d["dens"].shape == (50, P + 1) and d["counts"].shape == (10, P + 1)
        assert d["range"].shape == (2, P + 1) and d["bw"].shape == (P + 1,)
        th = chain_theta(ch, N, np.arange(301))
        want = lk.chaindens(th, ch["s2chain"][299:], **opt)
        for f, a, b in (("dens", want.dens, want.s2_dens), ("counts", want.counts, want.s2_counts),
                        ("range", want.range, want.s2_range), ("grid", want.grid(), want.s2_grid())):
            assert d[f][:, :P].tobytes() == np.ascontiguousarray(a[0]).tobytes(), f
            assert d[f][:, P].tobytes() == np.ascontiguousarray(b[0]).tobytes(), f
        assert d["bw"][:P].tobytes() == want.bw[0].tobytes() and d["bw"][P] == want.s2_bw[0]
        assert np.all(d["counts"].sum(axis=0) == 301) and np.all(np.isfinite(d["dens"]))
    dflt = fit(lk, cells=IDS[:1], density=True, **kw)                      # True: the default options
    assert dflt.MCMCdens[0]["dens"].shape[0] == 100 and dflt.MCMCdens[0]["counts"].shape[0] == 20
    plain = fit(lk, cells=IDS, **kw)                  # a fit without it has none, and the same chains
    assert plain.MCMCdens is None
    assert plain.MCMCchain[1]["dR_chain"].tobytes() == fr.MCMCchain[1]["dR_chain"].tobytes()
    shard = fit(lk, cells=IDS[1:2], density=opt, **kw)   # a one-cell shard reproduces the full fit's bits
    for f in DENS_FIELDS[:-2]:
        assert shard.MCMCdens[0][f].tobytes() == fr.MCMCdens[1][f].tobytes(), f
