"""Posterior mean, covariance and correlation on the device (tci_chaincov.hip) against the longdouble
restatement of tests/chaincov_oracle.py, within bounds that are derived there (chaincov_oracle.check): cov
within (n + 8) 2^-52 sqrt(ref_ii ref_jj), corr within (n + 16) 2^-52, mean within 4 x 2^-53 relative. Then
the structure (bitwise symmetry, unit diagonal, NaN padding), special columns, the bitwise invariances
(other chains, a wider ld, groups through the scratch) and the sampler's device chain.

Largest errors seen on an MI355X over the shape grid, in units of the bound: cov 0.18, corr 0.11, mean 0.50."""
import functools
import math

import numpy as np
import pytest

import chaincov_oracle as O

pytestmark = pytest.mark.gpu

IDS = [0, 150, 298]   # three TestData cells of unequal length
SHAPES = [(7, [7, 7, 7]), (16, [16, 16, 16]), (23, [17, 17, 17]), (40, [33, 16, 1]), (130, [130, 129, 113])]


@pytest.fixture(scope="module")
def lk(cells):
    from transcriptioncycleinference_amd import Likelihood

    with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as L:
        yield L


@functools.lru_cache(maxsize=None)
def case(ld, rows, n_chains):
    """Seeded random-walk chains, their npar, and the restatement's table (computed once, never changed)."""
    npar = np.array(dict(SHAPES)[ld][:n_chains], np.int32)
    chain = O.walk_chain(1000 * ld + rows, rows, n_chains, ld, npar)
    want = O.table(chain, npar)
    for a in (chain, npar, *want.values()):
        a.setflags(write=False)
    return chain, npar, want


def same(a, b):
    return all(getattr(a, k).tobytes() == getattr(b, k).tobytes() for k in ("mean", "cov", "corr")) and a.n_rows == b.n_rows


@pytest.mark.parametrize("n_chains", [1, 3])
@pytest.mark.parametrize("rows", [2, 3, 5, 1001])
@pytest.mark.parametrize("ld", [s[0] for s in SHAPES])
def test_parity_and_structure(lk, ld, rows, n_chains):
    chain, npar, want = case(ld, rows, n_chains)
    cc = lk.chaincov(chain, npar)
    assert cc.n_rows == rows and cc.kernel_ms > 0
    worst = O.check(cc, want, rows, f"ld={ld} rows={rows} chains={n_chains} ")
    print(f"chaincov ld={ld} rows={rows} chains={n_chains}: errors / bound {worst}")
    # structure: symmetric bit for bit, unit diagonal, NaN padding
    assert cc.cov.tobytes() == np.ascontiguousarray(np.transpose(cc.cov, (0, 2, 1))).tobytes()
    assert cc.corr.tobytes() == np.ascontiguousarray(np.transpose(cc.corr, (0, 2, 1))).tobytes()
    for c in range(n_chains):
        P = int(npar[c])
        assert np.all(np.diagonal(cc.corr[c])[:P] == 1.0) and np.all(np.diagonal(cc.cov[c])[:P] > 0)
        assert np.all(np.isfinite(cc.cov[c, :P, :P])) and np.all(np.abs(cc.corr[c, :P, :P]) <= 1.0)
        assert np.all(np.isnan(cc.mean[c, P:])) and np.all(np.isfinite(cc.mean[c, :P]))
        for a in (cc.cov[c], cc.corr[c]):
            assert np.all(np.isnan(a[P:, :])) and np.all(np.isnan(a[:, P:]))
    if ld >= 3 and rows >= 5 and npar[0] >= 3:
        assert cc.corr[0, 1, 2] < -0.99           # the column built next to -2 x its neighbour


def test_without_npar_every_column_is_real(lk):
    chain, _, _ = case(23, 5, 3)
    cc = lk.chaincov(chain)
    O.check(cc, O.table(chain), 5, "no npar ")
    assert np.all(np.isfinite(cc.cov)) and np.all(np.isfinite(cc.mean))
    one = lk.chaincov(chain[:, 1, :])             # a 2-D chain is one chain
    assert one.cov.shape == (1, 23, 23) and one.cov[0].tobytes() == cc.cov[1].tobytes()


def test_special_columns(lk):
    rows, ld = 257, 20
    chain = O.walk_chain(9, rows, 2, ld, [18, 20]).copy()
    chain[:, 0, 3] = 3.0            # constant
    chain[:, 0, 5] = 0.1            # a constant that is not a binary fraction
    chain[100, 0, 6] = np.nan       # one NaN
    chain[7, 0, 17] = np.inf        # one Inf, in the second tile
    npar = np.array([18, 20], np.int32)
    want = O.table(chain, npar)
    cc = lk.chaincov(chain, npar)
    O.check(cc, want, rows, "special ")
    bad, const = [6, 17], [3, 5]
    good = [j for j in range(18) if j not in bad + const]
    for j in bad:                   # poisons exactly its mean, row and column
        assert math.isnan(cc.mean[0, j])
        for a in (cc.cov[0], cc.corr[0]):
            assert np.all(np.isnan(a[j, :])) and np.all(np.isnan(a[:, j]))
    for a in (cc.cov[0], cc.corr[0]):
        assert np.all(np.isfinite(a[np.ix_(good, good)]))
    for j in const:                 # cov 0 against every finite column, corr 0/0
        assert cc.mean[0, j] == chain[0, 0, j]
        assert np.all(cc.cov[0, j, good + const] == 0.0) and np.all(cc.cov[0, good + const, j] == 0.0)
        assert np.all(np.isnan(cc.corr[0, j, :])) and np.all(np.isnan(cc.corr[0, :, j]))
    assert np.all(np.isfinite(cc.cov[1])) and np.all(np.isfinite(cc.corr[1]))   # the other chain is untouched


def test_bits_do_not_depend_on_the_layout(lk):
    """An element's bits depend on its two columns, their indices and n alone."""
    chain, npar, _ = case(40, 1001, 3)
    full = lk.chaincov(chain, npar)
    # chains [0, 2] alone
    two = lk.chaincov(np.ascontiguousarray(chain[:, [0, 2], :]), npar[[0, 2]])
    for k in ("mean", "cov", "corr"):
        assert getattr(two, k).tobytes() == np.ascontiguousarray(getattr(full, k)[[0, 2]]).tobytes(), k
    # the same columns in a wider ld
    wide = np.zeros((1001, 3, 57))
    wide[:, :, :40] = chain
    w = lk.chaincov(wide, npar)
    for c in range(3):
        P = int(npar[c])
        assert w.mean[c, :P].tobytes() == full.mean[c, :P].tobytes()
        for k in ("cov", "corr"):
            assert np.ascontiguousarray(getattr(w, k)[c, :P, :P]).tobytes() == \
                np.ascontiguousarray(getattr(full, k)[c, :P, :P]).tobytes(), k
        assert np.all(np.isnan(w.cov[c, P:, :])) and np.all(np.isnan(w.corr[c, :, P:]))
    # one chain per group through the scratch
    assert same(lk.chaincov(chain, npar, scratch_bytes=2 * 40 * 40 * 8), full)
    assert same(lk.chaincov(chain, npar, scratch_bytes=2 * 2 * 40 * 40 * 8 + 8), full)   # groups of 2 and 1


def test_bad_arguments_are_refused(lk):
    from transcriptioncycleinference_amd import TciError, _lib

    x = np.zeros((30, 2, 4))
    for chain, kw, code in ((x[:1], {}, _lib.TCI_EINVAL),                                   # n_rows = 1
                            (x, dict(npar=[5, 1]), _lib.TCI_ERANGE),                        # npar > ld
                            (x, dict(npar=[-1, 1]), _lib.TCI_ERANGE),
                            (x, dict(scratch_bytes=4 * 4 * 8 - 8), _lib.TCI_EINVAL),        # smaller than one matrix
                            (x, dict(scratch_bytes=2 * 4 * 4 * 8 - 8), _lib.TCI_EINVAL),    # ... than a chain's two
                            (x, dict(scratch_bytes=-1), _lib.TCI_EINVAL)):
        with pytest.raises(TciError) as e:
            lk.chaincov(chain, **kw)
        assert e.value.code == code, kw
    assert lk.chaincov(x[:2]).n_rows == 2          # and the context still works


# ---- tci_dram_run_cov: the matrices of the device chain ----------------------------------------------

def _plan(lk):
    from transcriptioncycleinference_amd.mcmc import plan_fit

    p = plan_fit(lk.cells, IDS, 3)
    return (np.array(IDS, np.int32), p.x0, p.lower, p.upper, p.prior_mu, p.prior_sig, p.qcov_diag, 1.0)


def _opts(**kw):
    from transcriptioncycleinference_amd.mcmc import DramOptions

    return DramOptions(n_steps=600, burnintime=200, adaptint=100, stats_from=300, thin=1, seed=19, **kw)


STAT_KEYS = ("mcerr", "tau", "tau_window", "geweke_z", "geweke_p", "s2_mcerr", "s2_tau", "s2_tau_window",
             "s2_geweke_z", "s2_geweke_p")


@pytest.mark.parametrize("engine", ["fused", "batched", "walk"])
def test_dram_matrices_equal_chaincov_of_the_returned_rows(lk, engine):
    from transcriptioncycleinference_amd.mcmc import dram_run

    npar = (7 + lk.cells.lengths[IDS]).astype(np.int32)
    res = dram_run(lk, *_plan(lk), _opts(engine=engine), cov=True)
    assert res.cov.n_rows == 301 and res.stats is None                  # rows 300 .. 600
    host = lk.chaincov(res.chain[299:], npar)
    assert same(res.cov, host)
    O.check(res.cov, O.table(res.chain[299:], npar), 301, f"dram {engine} ")
    # without the host chain, and with the chain statistics alongside
    both = dram_run(lk, *_plan(lk), _opts(engine=engine), cov=True, stats=True, want_chain=False)
    assert both.chain is None and both.s2chain is None and same(both.cov, host)
    alone = dram_run(lk, *_plan(lk), _opts(engine=engine), stats=True)
    assert alone.cov is None and both.stats.n_rows == alone.stats.n_rows == 301
    for k in STAT_KEYS:
        assert getattr(both.stats, k).tobytes() == getattr(alone.stats, k).tobytes(), k
    assert alone.chain.tobytes() == res.chain.tobytes() and alone.mean.tobytes() == both.mean.tobytes()


def test_dram_covariance_refusals(lk):
    from transcriptioncycleinference_amd import TciError, _lib
    from transcriptioncycleinference_amd.mcmc import DramOptions, dram_run

    ld = _plan(lk)[1].shape[1]
    for o, kw in ((DramOptions(n_steps=100, burnintime=50, stats_from=50, thin=0), {}),              # thin == 0
                  (DramOptions(n_steps=100, burnintime=50, stats_from=100, thin=1), {}),             # one row in range
                  (DramOptions(n_steps=100, burnintime=50, stats_from=50, thin=1),
                   dict(cov_scratch_bytes=ld * ld * 8 - 8))):                                        # below one matrix
        with pytest.raises(TciError) as e:
            dram_run(lk, *_plan(lk), o, cov=True, **kw)
        assert e.value.code == _lib.TCI_EINVAL
    # thinned: kept rows 1, 8, 15, ..; the first at or past row 50 is row 50 = 1 + 7 * 7
    o = DramOptions(n_steps=300, burnintime=100, stats_from=50, thin=7, seed=2)
    res = dram_run(lk, *_plan(lk), o, cov=True, cov_scratch_bytes=2 * ld * ld * 8)
    assert res.cov.n_rows == 43 - 7
    npar = (7 + lk.cells.lengths[IDS]).astype(np.int32)
    assert same(lk.chaincov(res.chain[7:], npar), res.cov)


# ---- fit(..., covariance=True) -----------------------------------------------------------------------

def test_fit_covariance(lk):
    from transcriptioncycleinference_amd.mcmc import COV_FIELDS, chain_theta, fit

    kw = dict(n_steps=600, n_burn=300, seed=4, thin=1)
    fr = fit(lk, cells=IDS, covariance=True, **kw)
    assert [d["cell_index"] for d in fr.MCMCcov] == [c + 1 for c in IDS] and fr.MCMCdiag is None
    for d, ch, c in zip(fr.MCMCcov, fr.MCMCchain, IDS):
        N = int(lk.cells.lengths[c])
        n = d["n_rows"]
        assert tuple(d) == COV_FIELDS and n == 301 == len(ch["v_chain"])
        assert d["cov"].shape == (7 + N, 7 + N) == d["corr"].shape and d["mean"].shape == (7 + N,)
        assert np.all(np.isfinite(d["cov"])) and np.all(np.diagonal(d["corr"]) == 1.0)
        th = chain_theta(ch, N, np.arange(n))
        sd = np.sqrt(np.diagonal(d["cov"]) * (n - 1) / n)
        assert np.max(np.abs(sd - th.std(axis=0)) / th.std(axis=0)) <= 1e-12
        assert np.max(np.abs(d["mean"] - th.mean(axis=0)) / np.max(np.abs(th), axis=0)) <= 1e-12
        assert d["cov"].tobytes() == lk.chaincov(th).cov[0].tobytes()
    plain = fit(lk, cells=IDS, **kw)                  # a fit without it has none, and the same chains
    assert plain.MCMCcov is None
    assert plain.MCMCchain[1]["dR_chain"].tobytes() == fr.MCMCchain[1]["dR_chain"].tobytes()
    shard = fit(lk, cells=IDS[1:2], covariance=True, **kw)   # a shard reproduces the full fit's bits
    assert shard.MCMCcov[0]["cov"].tobytes() == fr.MCMCcov[1]["cov"].tobytes()
    assert shard.MCMCcov[0]["corr"].tobytes() == fr.MCMCcov[1]["corr"].tobytes()
