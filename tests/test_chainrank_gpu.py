"""The rank diagnostics on the device (tci_chainrank.hip). Without tolerance: the pooled quantiles and every
central-branch z against the numpy restatement; rhat_bulk / ess_bulk / tau_bulk / window_bulk against tci_chainrhat /
tci_chainess run on the returned z; rhat_folded on the returned z_folded; the tail ESS on indicator chains built here
from the returned pooled quantiles; rhat_rank and ess_tail as the max and the min. Tail-branch z within
chainrank_oracle.Z_TAIL_ULP of the library's, on every element.

Shapes: N at the LDS cap - 1, the cap and the cap + 1 (both sort paths and their boundary), a three-tile global sort of
an N that is no power of two, N = 2, 3, 5, 63, 64, 65, M in {1, 2, 5} with n odd and even, interleaved groups of
different sizes with a chain of no group and unused ids, ld > npar, with and without s2; the tie shapes; the
independence of one group's bits from the layout; the samplers' own reductions; three statistical cases."""
import ctypes as C

import numpy as np
import pytest

import chainrank_oracle as O
from test_chainrank_host import sanity_chains

pytestmark = pytest.mark.gpu

IDS = [3, 41]            # two TestData cells
GROUP_FIELDS = ("q", "q_tail", "rhat_bulk", "rhat_folded", "rhat_rank", "ess_bulk", "tau_bulk", "ess_tail_lo",
                "ess_tail_hi", "ess_tail", "window_bulk", "window_tail_lo", "window_tail_hi")
worst_tail = {"ulp": 0.0}


@pytest.fixture(scope="module")
def lk(cells):
    from transcriptioncycleinference_amd import Likelihood

    with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
        yield lk


@pytest.fixture(scope="module", autouse=True)
def report_worst_tail():
    """One line after the module's last test: the largest tail-branch difference over every element it compared."""
    yield
    print(f"\nlargest tail-branch |z - library| over the whole module: {worst_tail['ulp']:.2f} ulp (bound {O.Z_TAIL_ULP})")


@pytest.fixture(scope="module")
def cap(lk):
    return int(lk._lib.tci_chainrank_lds_cap())


def bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def same(a, b):
    return a.n_rows == b.n_rows and all(bits(getattr(a, p + k), getattr(b, p + k)) for k in GROUP_FIELDS for p in ("", "s2_"))


def check_scores(got_z, ref_z, ref_p, where):
    """Central-branch scores bit for bit, tail-branch scores within the derived bound, NaN where the oracle has NaN."""
    nan = np.isnan(ref_z)
    assert np.array_equal(np.isnan(got_z), nan), where
    cen = ~nan & O.central(ref_p)
    assert bits(got_z[cen], ref_z[cen]), where
    tail = ~nan & ~cen
    if tail.any():
        d = float(np.max(O.ulp_diff(got_z[tail], ref_z[tail])))
        worst_tail["ulp"] = max(worst_tail["ulp"], d)
        assert d <= O.Z_TAIL_ULP, (where, d)
    return int(cen.sum()), int(tail.sum())


def check_case(lk, chain, s2=None, npar=None, group=None, probs=(0.025, 0.5, 0.975), tail=(0.05, 0.95), max_lag=0,
               where=""):
    chain = np.ascontiguousarray(chain, np.float64)
    n, nc, ld = chain.shape
    got = lk.chainrank(chain, s2, npar, group, probs=probs, tail=tail, max_lag=max_lag, scores=True)
    ref = O.table(chain, s2, npar, group, probs=probs, tail=tail, stats=False)
    assert got.n_rows == n
    # exact: the pooled quantiles
    assert bits(O.joined(got, "q"), ref["q"]) and bits(O.joined(got, "q_tail"), ref["q_tail"]), where
    # the scores
    counts = check_scores(O.joined_chain(got.z, got.s2_z), ref["z"], ref["p"], (where, "z"))
    check_scores(O.joined_chain(got.z_folded, got.s2_z_folded), ref["z_folded"], ref["p_folded"], (where, "z_folded"))
    # exact: the split statistics are tci_chainrhat's / tci_chainess's of the returned chains
    rb = lk.chainrhat(got.z, got.s2_z, npar, group)
    eb = lk.chainess(got.z, got.s2_z, npar, group, max_lag=max_lag)
    for p in ("", "s2_"):
        assert bits(getattr(got, p + "rhat_bulk"), getattr(rb, p + "rhat_split")), where
        assert bits(getattr(got, p + "ess_bulk"), getattr(eb, p + "ess_split")), where
        assert bits(getattr(got, p + "tau_bulk"), getattr(eb, p + "tau_split")), where
        assert bits(getattr(got, p + "window_bulk"), getattr(eb, p + "window_split")), where
    rf = lk.chainrhat(got.z_folded, got.s2_z_folded, npar, group)
    assert bits(got.rhat_folded, rf.rhat_split) and bits(got.s2_rhat_folded, rf.s2_rhat_split), where
    # the indicator chains, built here from the returned pooled quantiles
    x = np.full((n, nc, ld + 1), np.nan)
    x[:, :, :ld] = chain
    if s2 is not None:
        x[:, :, ld] = s2
    grp = np.zeros(nc, np.int64) if group is None else np.asarray(group)
    qt = O.joined(got, "q_tail")
    for t, name in enumerate(("lo", "hi")):
        ind = np.full_like(x, np.nan)
        for g in range(qt.shape[0]):
            cs = np.nonzero(grp == g)[0]
            q = qt[g, t]
            ind[:, cs, :] = np.where(np.isnan(q), np.nan, (x[:, cs, :] <= q).astype(np.float64))
        et = lk.chainess(np.ascontiguousarray(ind[:, :, :ld]), ind[:, :, ld] if s2 is not None else None, npar, group,
                         max_lag=max_lag)
        for p in ("", "s2_"):
            assert bits(getattr(got, p + "ess_tail_" + name), getattr(et, p + "ess_split")), (where, name)
            assert bits(getattr(got, p + "window_tail_" + name), getattr(et, p + "window_split")), (where, name)
    with np.errstate(invalid="ignore"):
        for p in ("", "s2_"):
            a, b = getattr(got, p + "rhat_bulk"), getattr(got, p + "rhat_folded")
            assert bits(getattr(got, p + "rhat_rank"), np.where(np.isnan(a) | np.isnan(b), np.nan, np.maximum(a, b))), where
            a, b = getattr(got, p + "ess_tail_lo"), getattr(got, p + "ess_tail_hi")
            assert bits(getattr(got, p + "ess_tail"), np.where(np.isnan(a) | np.isnan(b), np.nan, np.minimum(a, b))), where
    return got, counts


def dram_like(rng, n, nc, ld, accept=0.2):
    """Chains that repeat their rows as a sampler with `accept` acceptance does: every value appears several times."""
    moves = rng.random((n, nc, 1)) < accept
    moves[0] = True
    idx = np.maximum.accumulate(np.where(moves, np.arange(n)[:, None, None], 0), axis=0)
    fresh = rng.standard_normal((n, nc, ld))
    return np.ascontiguousarray(np.take_along_axis(fresh, np.broadcast_to(idx, fresh.shape), axis=0))


def test_both_sort_paths_and_their_boundary(lk, cap):
    rng = np.random.default_rng(21)
    for N in (cap - 1, cap, cap + 1):
        x = dram_like(rng, N, 1, 1)
        _, (cen, tl) = check_case(lk, x, max_lag=40, where=f"N{N}")
        assert cen > 0 and tl > 0
    # three tiles in global memory, N no power of two, M = 3 with an odd n, with s2
    n = (2 * cap + 39) // 3
    x = dram_like(rng, n, 3, 2)
    check_case(lk, x, s2=np.abs(dram_like(rng, n, 3, 1))[:, :, 0] + 0.5, max_lag=40, where="three tiles")


def test_small_and_odd_shapes(lk):
    rng = np.random.default_rng(22)
    for n in (2, 3, 5, 63, 64, 65):
        check_case(lk, rng.standard_normal((n, 1, 2)), where=f"n{n}")
    for M, n in ((2, 33), (2, 34), (5, 13), (5, 14)):
        check_case(lk, rng.standard_normal((n, M, 3)), s2=rng.random((n, M)) + 0.1, where=f"M{M}n{n}")
    # interleaved groups of sizes 3, 4 and 1, a chain of no group, ids 1 and 3 unused, ld above npar, with and without s2
    group = np.array([0, 2, 0, -1, 2, 2, 4, 0, 2], np.int32)
    x = dram_like(rng, 37, 9, 6)
    x[:, :, 4:] = np.nan  # padding is never read
    for s2 in (None, rng.random((37, 9)) + 0.1):
        got, _ = check_case(lk, x, s2=s2, npar=np.full(9, 4, np.int32), group=group, probs=(0.0, 0.3, 1.0), tail=(0.1, 0.8),
                            where="interleaved")
        assert got.q.shape == (5, 3, 6) and np.all(np.isnan(got.q[[1, 3]])) and np.all(np.isnan(got.q[:, :, 4:]))
        assert np.all(np.isnan(got.z[:, 3])) and np.all(np.isnan(got.z[:, :, 4:])) and np.all(np.isfinite(got.z[:, 0, :4]))
        assert np.all(got.window_bulk[[1, 3]] == -1) and np.all(got.window_bulk[:, 4:] == -1)
        assert np.all(np.isfinite(got.rhat_rank[[0, 2, 4], :4]))
        if s2 is None:
            assert all(np.all(np.isnan(getattr(got, "s2_" + k))) for k in GROUP_FIELDS[:10])
            assert all(np.all(getattr(got, "s2_" + k) == -1) for k in GROUP_FIELDS[10:])
        else:
            assert np.all(np.isfinite(got.s2_rhat_rank[[0, 2, 4]])) and np.all(np.isnan(got.s2_rhat_rank[[1, 3]]))


def tie_chain(rng, n=200, M=3):
    x = np.empty((n, M, 8))
    runs = np.repeat(rng.standard_normal(n), rng.integers(3, 41, n))[:n * M]
    runs[-3:] = runs[-4]
    x[:, :, 0] = runs.reshape(M, n).T                                   # every value 3 to 40 times or so
    x[:, :, 1] = 1.25
    x[17, 1, 1] = -3.0                                                  # one value except for one element
    x[:, :, 2] = 2.5                                                    # constant
    x[:, :, 3] = np.where(rng.random((n, M)) < 0.5, 0.0, -0.0)          # -0 and +0 mixed
    u = rng.random((n, M))
    x[:, :, 4] = np.where(u < 0.4, 0.0, np.where(u > 0.7, 1.0, u))      # values at both box bounds
    x[:, :, 5] = rng.standard_normal((n, M))
    x[3, 2, 5] = np.nan
    x[:, :, 6] = rng.standard_normal((n, M))
    x[9, 0, 6] = np.inf
    x[:, :, 7] = rng.choice([5e-324, -5e-324, 1e-310, 1e300, -1e300, 0.5], (n, M))  # denormals and +-1e300
    return x


def test_tie_shapes(lk):
    rng = np.random.default_rng(23)
    x = tie_chain(rng)
    counts = np.unique(x[:, :, 0], return_counts=True)[1]
    assert counts.min() >= 3 and counts.max() <= 60
    s2 = np.round(rng.random((200, 3)), 1) + 0.1
    got, _ = check_case(lk, x, s2=s2, where="ties")
    assert np.all(got.z[:, :, 2] == 0.0) and np.isnan(got.rhat_rank[0, 2]) and np.isnan(got.ess_bulk[0, 2])
    assert got.q[0, 1, 2] == 2.5
    for j in (5, 6):
        assert np.all(np.isnan(got.z[:, :, j])) and np.all(np.isnan(got.q[0, :, j])) and np.isnan(got.ess_tail[0, j])
        assert got.window_bulk[0, j] == got.window_tail_lo[0, j] == got.window_tail_hi[0, j] == -1
    lo = got.z[:, :, 3][np.signbit(x[:, :, 3])]
    assert np.all(lo == lo[0]) and np.all(lo < 0) and np.all(got.z[:, :, 3][~np.signbit(x[:, :, 3])] > 0)
    assert np.isfinite(got.rhat_rank[0, 7]) and np.isfinite(got.ess_tail[0, 0])


def test_one_group_has_the_same_bits_wherever_it_sits(lk):
    rng = np.random.default_rng(24)
    n, M = 61, 3
    mine = dram_like(rng, n, M, 3)
    s2m = rng.random((n, M)) + 0.2
    alone = lk.chainrank(mine, s2m, max_lag=9)
    # in a batch of 7 groups, at another ld, its chains scattered
    nc, ld = 16, 7
    batch = rng.standard_normal((n, nc, ld))
    s2 = rng.random((n, nc)) + 0.2
    group = np.array([1, 5, 0, 3, 5, 2, 4, 3, 6, 5, 1, 0, -1, 6, 2, 4], np.int32)
    where = np.nonzero(group == 5)[0]
    batch[:, where, :3], s2[:, where] = mine, s2m
    npar = np.where(group == 5, 3, 7).astype(np.int32)
    npar[group == 3] = 5
    both = lk.chainrank(batch, s2, npar, group, max_lag=9)
    for k in GROUP_FIELDS:
        assert bits(getattr(both, k)[5][..., :3], getattr(alone, k)[0]), k
        assert bits(getattr(both, "s2_" + k)[5], getattr(alone, "s2_" + k)[0]), k


def _opts(**kw):
    from transcriptioncycleinference_amd.mcmc import DramOptions

    return DramOptions(**{**dict(n_steps=400, burnintime=100, stats_from=100, thin=1, seed=7), **kw})


def test_the_dram_reduction_is_chainrank_of_the_chain_handed_back(lk):
    from transcriptioncycleinference_amd.mcmc import dram_run, plan_fit, replicate_keys

    p = plan_fit(lk.cells, IDS, 11, replicates=3)
    plan = (np.tile(np.array(IDS, np.int32), 3), p.x0, p.lower, p.upper, p.prior_mu, p.prior_sig, p.qcov_diag, 1.0)
    group = np.tile(np.arange(2, dtype=np.int32), 3)
    keys = replicate_keys(IDS, 3)
    npar = (7 + lk.cells.lengths[np.tile(IDS, 3)]).astype(np.int32)
    first = None
    for engine in ("fused", "batched", "walk"):
        res = dram_run(lk, *plan, _opts(engine=engine), chain_keys=keys, group=group, rank=True, max_lag=50)
        assert res.rank.n_rows == 301
        host = lk.chainrank(res.chain[99:], res.s2chain[99:], npar, group, max_lag=50)
        assert same(res.rank, host), engine
        first = first or res
        assert same(res.rank, first.rank), engine
    P = 7 + int(lk.cells.lengths[3])
    assert np.all(np.isfinite(first.rank.q[0, :, :P])) and np.all(first.rank.window_bulk[0, :P] >= 0)
    # kout = NULL leaves every existing output as it was
    plain = dram_run(lk, *plan, _opts(engine="fused"), chain_keys=keys, group=group, ess=True, max_lag=50)
    with_rank = dram_run(lk, *plan, _opts(engine="fused"), chain_keys=keys, group=group, ess=True, rank=True, max_lag=50)
    assert bits(plain.chain, with_rank.chain) and bits(plain.s2chain, with_rank.s2chain) and bits(plain.mean, with_rank.mean)
    for k in ("ess", "ess_split", "tau", "tau_split", "mcse", "window", "window_split", "s2_ess"):
        assert bits(getattr(plain.ess, k), getattr(with_rank.ess, k)), k
    for k in ("rhat", "rhat_split", "pooled_mean", "pooled_std"):
        assert bits(getattr(plain.rhat, k), getattr(with_rank.rhat, k)), k
    assert same(with_rank.rank, first.rank)
    with pytest.raises(ValueError):
        dram_run(lk, *plan, _opts(), chain_keys=keys, rank=True)


def test_the_demc_reduction_is_chainrank_of_the_chain_handed_back(lk):
    from transcriptioncycleinference_amd import mcmc

    sp = mcmc.search_population(lk.cells, [IDS[0]], 5, 5)
    jit = np.zeros_like(sp.lower)
    j = mcmc.demc_jitter(lk.cells, sp.cells)
    jit[:, :j.shape[1]] = j
    run = lambda **kw: lk.demc(sp.pop0, np.array(sp.cells, np.int32), sp.lower, sp.upper, sp.prior_mu, sp.prior_sig, jit,  # noqa: E731
                               seed=5, n_gen=60, thin=1, stats_from=10, rhat=True, ess=True, max_lag=20, **kw)
    plain, ranked = run(), run(rank=dict(probs=(0.1, 0.5, 0.9)))
    assert plain.rank is None and ranked.rank.n_rows == 51
    assert bits(plain.chain, ranked.chain) and bits(plain.s2chain, ranked.s2chain) and bits(plain.pop, ranked.pop)
    for k in ("ess", "ess_split", "tau", "window"):
        assert bits(getattr(plain.ess, k), getattr(ranked.ess, k)), k
    assert bits(plain.rhat.rhat, ranked.rhat.rhat)
    P = 7 + int(lk.cells.lengths[IDS[0]])
    host = lk.chainrank(ranked.chain[10:], ranked.s2chain[10:], np.full(5, P, np.int32), np.zeros(5, np.int32),
                        probs=(0.1, 0.5, 0.9), max_lag=20)
    assert same(ranked.rank, host)


def test_statistical_cases(lk):
    got = lk.chainrank(sanity_chains("iid"))
    print("iid", got.rhat_rank[0, 0], got.ess_bulk[0, 0], got.ess_tail[0, 0])
    assert got.rhat_rank[0, 0] < 1.05 and 1000 <= got.ess_bulk[0, 0] <= 4000
    x = sanity_chains("scales")
    got = lk.chainrank(x)
    classic = lk.chainrhat(x).rhat[0, 0]
    print("scales", got.rhat_bulk[0, 0], got.rhat_folded[0, 0], classic)
    assert got.rhat_folded[0, 0] > 1.1 and got.rhat_folded[0, 0] > got.rhat_bulk[0, 0] + 0.05 and classic < 1.05
    got = lk.chainrank(sanity_chains("cauchy"))
    print("cauchy", got.rhat_rank[0, 0], got.ess_bulk[0, 0], got.ess_tail[0, 0])
    assert got.rhat_rank[0, 0] < 1.05 and 500 <= got.ess_bulk[0, 0] <= 4000 and 100 <= got.ess_tail[0, 0] <= 4000


def test_the_abi_refuses_bad_arguments_before_device_work(lk):
    from transcriptioncycleinference_amd import _lib
    from transcriptioncycleinference_amd.likelihood import ChainRank

    x = np.zeros((6, 3, 2))

    def call(rows=6, nc=3, ld=2, npar=None, group=None, ng=1, chain=x, o=True, **opt):
        ck = ChainRank.empty(max(ng, 1), ld)
        k, out = ck.options(), ck.to_c()
        for name, v in opt.items():
            if name == "prob0":
                k.probs[0] = v
            else:
                setattr(k, name, v)
        a = lambda v: None if v is None else np.ascontiguousarray(v, np.int32)  # noqa: E731
        npar_a, group_a = a(npar), a(group)
        rc = lk._lib.tci_chainrank(lk._h, C.byref(k), _lib.ptr(chain, _lib._dp), None, rows, nc, ld,
                                   _lib.ptr(npar_a, _lib._i32p), _lib.ptr(group_a, _lib._i32p), ng,
                                   C.byref(out) if o else None)
        return rc, lk._lib.tci_last_error(lk._h).decode()

    assert call()[0] == _lib.TCI_OK
    for kw in (dict(rows=0), dict(ng=0), dict(ng=4), dict(chain=None), dict(o=None), dict(nq=0), dict(nq=17),
               dict(prob0=1.5), dict(prob0=float("nan")), dict(tail_lo=0.0), dict(tail_hi=1.0), dict(tail_lo=0.96),
               dict(max_lag=-1), dict(flags=1), dict(nc=0), dict(ld=0), dict(npar=[2, 1, 2])):
        rc, msg = call(**kw)
        assert rc == _lib.TCI_EINVAL and msg.startswith("tci_chainrank"), (kw, msg)
    assert call(group=[0, 2, 0], ng=2)[0] == _lib.TCI_ERANGE
    assert call(group=[0, -2, 0], ng=2)[0] == _lib.TCI_ERANGE
    assert call(npar=[2, 3, 2])[0] == _lib.TCI_ERANGE
    # the options are checked after n_rows and before n_chains, as tci_chainess checks its own
    assert "n_rows" in call(rows=0, flags=1)[1] and "flags" in call(flags=1, nc=0)[1]
