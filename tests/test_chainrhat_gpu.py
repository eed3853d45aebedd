"""The group reduction on the device (tci_chainrhat.hip): against the longdouble restatement within the derived
bound at the shapes where the kernels can go wrong, the special columns, the invariance of an output's bits to the
layout, the run's own reduction against the chain it hands back, and fit(..., replicates=M)."""
import ctypes as C

import numpy as np
import pytest

import chainrhat_oracle as O

pytestmark = pytest.mark.gpu

IDS = [3, 41, 120]       # three TestData cells


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
                                        for k in O.OUTPUTS for p in ("", "s2_"))


def test_every_shape_and_special_column_within_the_bound(lk, cases):
    """n on both sides of the 8 / 32-row step and of the 256-row segment, every ld around the 64-column tile, M from 1
    to 7, ragged npar, interleaved and descending groups, chains of no group, with and without s2; then the special
    columns and the offset fixture. Prints how far the device stayed inside the bound."""
    worst_all = 0.0
    for c in cases:
        ref = O.table(c["chain"], c["s2"], c["npar"], c["group"], dtype=O.LD)
        got = lk.chainrhat(c["chain"], c["s2"], c["npar"], c["group"])
        assert got.n_rows == c["n"]
        worst, _ = O.check(O.joined(got), ref, c["n"], where=c["name"])
        print(f"{c['name']}: largest error / bound {max(worst.values()):.3f}")
        worst_all = max(worst_all, max(worst.values()))
        if c["s2"] is None:
            assert all(np.all(np.isnan(getattr(got, "s2_" + k))) for k in O.OUTPUTS)
    print(f"largest error as a fraction of the bound over all fixtures: {worst_all:.3f}")


def test_identical_chains_and_the_special_columns_exactly(lk, cases):
    sp = next(c for c in cases if c["name"] == "special")
    got = lk.chainrhat(sp["chain"], sp["s2"], sp["npar"], sp["group"])
    assert got.rhat[0, 6] == np.sqrt(np.float64(299) / np.float64(300))
    assert np.isnan(got.rhat[0, 1]) and got.pooled_mean[0, 1] == 2.5 and got.pooled_std[0, 1] == 0.0
    assert np.isposinf(got.rhat[0, 3]) and np.isposinf(got.rhat_split[0, 3])
    for M in (2, 3, 4, 7):
        one = sp["chain"][:257, :1, :1]
        rep = lk.chainrhat(np.repeat(one, M, axis=1))
        assert rep.rhat[0, 0] == np.sqrt(np.float64(256) / np.float64(257)), M
        assert rep.pooled_mean.tobytes() == lk.chainrhat(one).pooled_mean.tobytes()


def test_bits_do_not_depend_on_the_layout(lk):
    """An output's bits depend on the group's columns in chain order and on n alone."""
    n, M, ld = 513, 3, 37
    npar = np.full(M, 33, np.int32)
    chain, s2 = O.walk_chains(9, n, M, ld, npar)
    alone = lk.chainrhat(chain, s2, npar)
    others, s2o = O.walk_chains(10, n, 40, 70, np.full(40, 70))
    # among 40 other chains, at a wider ld, the group's chains apart but in order, the others in groups of their own
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
        got = lk.chainrhat(big, big_s2, bnpar, group)
        for k in O.OUTPUTS:
            assert getattr(got, k)[mine, :ld].tobytes() == getattr(alone, k)[0].tobytes(), (mine, k)
            assert getattr(got, "s2_" + k)[mine] == getattr(alone, "s2_" + k)[0], (mine, k)
            assert np.all(np.isnan(getattr(got, k)[mine, 33:]))
    # the chains of a group in another order are another statistic only in the last bits: same within the bound
    ref = O.table(chain, s2, npar, dtype=O.LD)
    O.check(O.joined(lk.chainrhat(chain[:, ::-1], s2[:, ::-1], npar)), ref, n, "reversed chains")


def test_bad_arguments_are_refused(lk):
    from transcriptioncycleinference_amd import _lib

    x = np.zeros((20, 3, 2))
    out = _lib.tci_chainrhat_outputs()
    P, I = (lambda a: _lib.ptr(a, _lib._dp)), (lambda a: _lib.ptr(np.ascontiguousarray(a, np.int32), _lib._i32p))  # noqa: E731

    def call(opt=None, rows=20, npar=None, group=None, ng=1, chain=x, o=out):
        rc = lk._lib.tci_chainrhat(lk._h, None if opt is None else C.byref(opt), P(chain), None, rows, 3, 2,
                                   None if npar is None else I(npar), None if group is None else I(group), ng,
                                   None if o is None else C.byref(o))
        return rc, lk._lib.tci_last_error(lk._h).decode()

    assert call()[0] == _lib.TCI_OK
    rc, msg = call(opt=_lib.tci_chainrhat_options(1))
    assert rc == _lib.TCI_EINVAL and "flags" in msg
    rc, msg = call(npar=[2, 1, 2], group=[1, 0, 0], ng=2)
    assert rc == _lib.TCI_EINVAL and "group 0" in msg and "npar" in msg
    assert call(npar=[2, 1, 2], group=[0, 1, 0], ng=2)[0] == _lib.TCI_OK
    assert call(group=[0, 2, 0], ng=2)[0] == _lib.TCI_ERANGE
    assert call(group=[0, -2, 0], ng=2)[0] == _lib.TCI_ERANGE
    assert call(npar=[2, 3, 2])[0] == _lib.TCI_ERANGE
    for kw in (dict(rows=0), dict(ng=0), dict(ng=4), dict(chain=None), dict(o=None)):
        assert call(**kw)[0] == _lib.TCI_EINVAL, kw
    # a group id no chain carries: NaN, not an error
    got = lk.chainrhat(x + np.arange(20)[:, None, None], group=np.array([2, 0, 2]))
    assert np.all(np.isnan(got.rhat[1])) and np.all(np.isnan(got.pooled_mean[1])) and np.all(np.isfinite(got.rhat[2]))


def _opts(**kw):
    from transcriptioncycleinference_amd.mcmc import DramOptions

    return DramOptions(**{**dict(n_steps=600, burnintime=200, stats_from=200, thin=1, seed=7), **kw})


def _plan(lk, replicates=1):
    from transcriptioncycleinference_amd.mcmc import plan_fit

    p = plan_fit(lk.cells, IDS, 11, replicates=replicates)
    return (np.tile(np.array(IDS, np.int32), replicates), p.x0, p.lower, p.upper, p.prior_mu, p.prior_sig, p.qcov_diag,
            1.0)


def test_duplicate_chains_and_the_chain_handed_back(lk):
    """Two chains on one cell from one x0 on one RNG stream are the same chain: classic rhat is exactly
    sqrt((n - 1) / n) on every real column. The run's reduction equals chainrhat of the rows it returns."""
    from transcriptioncycleinference_amd.mcmc import dram_run

    cid, x0, lo, up, mu, sig, q, s20 = _plan(lk)
    dup = lambda a: np.concatenate([a, a[:1]])  # noqa: E731  (chain 3 = chain 0 again)
    keys = np.array([3, 41, 120, 3], np.int64)
    group = np.array([0, 1, -1, 0], np.int32)
    res = dram_run(lk, dup(cid), dup(x0), dup(lo), dup(up), dup(mu), dup(sig), dup(q), s20, _opts(), chain_keys=keys,
                   group=group)
    n = res.rhat.n_rows
    assert n == 401                                          # rows 200 .. 600
    assert res.chain[:, 0].tobytes() == res.chain[:, 3].tobytes()
    P = 7 + int(lk.cells.lengths[3])
    want = np.sqrt(np.float64(n - 1) / np.float64(n))
    assert np.all(res.rhat.rhat[0, :P] == want) and res.rhat.s2_rhat[0] == want
    assert np.all(np.isnan(res.rhat.rhat[0, P:])) and np.all(np.isnan(res.rhat.rhat[1]))   # group 1: one chain
    assert np.all(np.isfinite(res.rhat.rhat_split[1, :7 + int(lk.cells.lengths[41])]))
    npar = (7 + lk.cells.lengths[dup(cid)]).astype(np.int32)
    host = lk.chainrhat(res.chain[199:], res.s2chain[199:], npar, group)
    assert same(res.rhat, host)
    bare = dram_run(lk, dup(cid), dup(x0), dup(lo), dup(up), dup(mu), dup(sig), dup(q), s20, _opts(), chain_keys=keys,
                    group=group, want_chain=False)
    assert bare.chain is None and same(bare.rhat, host)


def test_replicate_keys_give_different_random_streams(lk):
    """Two chains on one cell from one x0 differ as soon as their keys differ modulo 2^32, which is what a replicate's
    key does; a key that differs above bit 32 alone is the same stream (include/tci.h, chain_keys), so the replicates
    of a cell would share every proposal, acceptance and sigma2 draw and R-hat would sit near 1 whatever the
    posterior."""
    from transcriptioncycleinference_amd.mcmc import dram_run, replicate_keys

    cid, x0, lo, up, mu, sig, q, s20 = _plan(lk)
    rep = lambda a: np.repeat(a[:1], 3, axis=0)  # noqa: E731  (cell 3 three times, one x0)
    keys = np.array([3, replicate_keys([3], 2)[1], 3 + 2**40], np.int64)
    assert keys[1] % 2**32 != 3
    res = dram_run(lk, rep(cid), rep(x0), rep(lo), rep(up), rep(mu), rep(sig), rep(q), s20, _opts(), chain_keys=keys,
                   group=np.array([0, 0, -1], np.int32))
    P = 7 + int(lk.cells.lengths[3])
    a, b, c = (np.ascontiguousarray(res.chain[:, k, :P]) for k in range(3))
    assert a.tobytes() == c.tobytes()                        # keys equal modulo 2^32: one stream
    moved = np.any(a[1:] != a[:-1], axis=1) | np.any(b[1:] != b[:-1], axis=1)
    assert moved.sum() > 50 and not np.any(np.all(a[1:] == b[1:], axis=1)[moved])   # the replicate's key: no move in common
    assert res.s2chain[:, 0].tobytes() != res.s2chain[:, 1].tobytes()
    assert np.all(res.rhat.rhat[0, :P] > np.sqrt(400.0 / 401.0))


def test_run_rhat_with_the_other_reductions_and_refusals(lk):
    """tci_dram_run_rhat with all four other reductions: they are what they are without it."""
    from transcriptioncycleinference_amd import TciError, _lib
    from transcriptioncycleinference_amd.mcmc import dram_run, replicate_keys

    plan = _plan(lk, 2)
    group = np.tile(np.arange(3, dtype=np.int32), 2)
    keys = replicate_keys(IDS, 2)
    kw = dict(stats=True, cov=True, quant=(0.025, 0.5, 0.975), dens=dict(n_grid=16, n_bins=8), chain_keys=keys,
              want_chain=False)
    a = dram_run(lk, *plan, _opts(), group=group, **kw)
    b = dram_run(lk, *plan, _opts(), **kw)
    only = dram_run(lk, *plan, _opts(), group=group, chain_keys=keys, want_chain=False)
    assert b.rhat is None and same(a.rhat, only.rhat) and only.stats is None and only.dens is None
    for red, fields in (("stats", ("mcerr", "tau", "geweke_z", "geweke_p", "tau_window", "s2_tau")),
                        ("cov", ("mean", "cov", "corr")), ("quant", ("q", "s2_q")),
                        ("dens", ("range", "bw", "dens", "counts", "s2_dens", "s2_counts"))):
        for f in fields:
            assert getattr(getattr(a, red), f).tobytes() == getattr(getattr(b, red), f).tobytes(), (red, f)
    for o in (_opts(thin=0), _opts(stats_from=600)):          # no kept rows; one row in range
        with pytest.raises(TciError) as e:
            dram_run(lk, *plan, o, group=group, chain_keys=keys)
        assert e.value.code == _lib.TCI_EINVAL
    with pytest.raises(TciError) as e:                        # cell 120 is shorter than cells 3 and 41: mixed npar
        dram_run(lk, *plan, _opts(), group=np.zeros(6, np.int32), chain_keys=keys)
    assert e.value.code == _lib.TCI_EINVAL and "group 0" in str(e.value)


def test_fit_replicates(lk):
    from transcriptioncycleinference_amd.mcmc import RHAT_FIELDS, DramOptions, dram_run, fit, replicate_keys

    kw = dict(n_steps=600, n_burn=200, thin=1, seed=11, cells=IDS, quantiles=(0.025, 0.5, 0.975))
    one = fit(lk, **kw)
    four = fit(lk, replicates=4, **kw)
    assert one.MCMCrhat is None and len(four.MCMCrhat) == 3

    def flat(x):
        if isinstance(x, dict):
            return b"".join(flat(x[k]) for k in sorted(x))
        return np.ascontiguousarray(x).tobytes()

    for name in ("MCMCresults", "MCMCchain", "MCMCquant", "MCMCplot"):
        for a, b in zip(getattr(one, name), getattr(four, name)):
            assert flat(a) == flat(b), name
    assert four.accept_rate.tobytes() == one.accept_rate.tobytes() and four.n_evals > 3 * one.n_evals
    assert four.final_theta.tobytes() == one.final_theta.tobytes()
    # MCMCrhat against chainrhat of all twelve chains (the run fit() makes, asked for its chain) and the oracle
    o = DramOptions(n_steps=600, burnintime=200, stats_from=200, thin=1, seed=11 * 1000003 + 20201028)
    keys = replicate_keys(IDS, 4)
    group = np.tile(np.arange(3, dtype=np.int32), 4)
    run = dram_run(lk, *_plan(lk, 4), o, chain_keys=keys)
    npar = (7 + lk.cells.lengths[np.tile(IDS, 4)]).astype(np.int32)
    host = lk.chainrhat(run.chain[199:], run.s2chain[199:], npar, group)
    ref = O.table(run.chain[199:], run.s2chain[199:], npar, group, dtype=O.LD)
    O.check(O.joined(host), ref, 401, "fit")
    for k, c in enumerate(IDS):
        e, P = four.MCMCrhat[k], 7 + int(lk.cells.lengths[c])
        assert tuple(e) == RHAT_FIELDS and e["n_rows"] == 401 and e["n_chains"] == 4 and e["cell_index"] == c + 1
        for f in O.OUTPUTS:
            assert e[f].tobytes() == np.concatenate([getattr(host, f)[k, :P], [getattr(host, "s2_" + f)[k]]]).tobytes()
        assert e["mean_rep"].shape == (4, P) and e["mean_rep"].tobytes() == np.ascontiguousarray(run.mean[k::3, :P]).tobytes()
        assert e["accept_rep"].tobytes() == np.ascontiguousarray(run.accept_rate[k::3]).tobytes()
        assert np.all(np.isfinite(e["rhat"])) and e["rhat_max"] >= 1.0 - 1.0 / 401
    # every engine: the same MCMCrhat
    for engine in ("fused", "batched", "walk"):
        other = fit(lk, replicates=4, opts=DramOptions(engine=engine), **kw)
        for a, b in zip(four.MCMCrhat, other.MCMCrhat):
            assert flat(a) == flat(b), engine
    # one replicate with rhat=True: the split factor alone
    solo = fit(lk, rhat=True, **kw)
    assert all(np.all(np.isnan(e["rhat"])) and np.all(np.isfinite(e["rhat_split"])) for e in solo.MCMCrhat)
    assert all(flat(a) == flat(b) for a, b in zip(one.MCMCchain, solo.MCMCchain))
