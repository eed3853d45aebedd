"""Parallel tempering on the device (tci_dram_run_tempered, include/tci.h; MI355X): the tempered call reduces to the
plain sampler bit for bit, the three engines agree, the swap follows the float64 restatement (tests/temper_oracle.py),
an accepted swap exchanges exactly the two states, the tempered sigma2 draw has its Gamma law and the cold rung of a
ladder samples the posterior a plain chain samples.

Shapes: two cells of 12 and 17 points (so ld is ragged), ladders of 2, 3 and 4 rungs with one chain outside any ladder
between them, adaptint = 20 and n_steps in {15, 100, 101}: no window end, a window end on the last row (four swap events,
none after row 100) and five swap events."""
import dataclasses

import numpy as np
import pytest

import temper_oracle as TO

pytestmark = pytest.mark.gpu

N_POINTS = (12, 17)
#          ladder 0 (2 rungs)  ladder 1 (3 rungs)  none  ladder 2 (4 rungs)
CELL = np.array([0, 0, 1, 1, 1, 1, 0, 0, 0, 0], np.int32)
LADDER = np.array([0, 0, 1, 1, 1, -1, 2, 2, 2, 2], np.int32)
PLAIN = 5
AI = 20


@pytest.fixture(scope="module")
def small(cells):
    from transcriptioncycleinference_amd.data import from_lists

    return from_lists([tuple(a[:n] for a in cells.cell(c)) for c, n in enumerate(N_POINTS)], "temper")


@pytest.fixture(scope="module")
def lk(small):
    from transcriptioncycleinference_amd import Likelihood

    with Likelihood(small, "P2P-MS2v5-LacZ-PP7v4", device=0) as L:
        yield L


def setup(small, cell_id, seed=0):
    """x0, lower, upper, mu, sig, J0 rows (padded to ld): bounds and priors are the cell's, x0 differs per chain."""
    from transcriptioncycleinference_amd.mcmc import cell_setup

    rng = np.random.default_rng(seed)
    rows = [cell_setup(small.cell(int(c))[0], rng, 50.0) for c in cell_id]
    ld = max(len(r[0]) for r in rows)
    out = []
    for i, fill in enumerate((0.0, -np.inf, np.inf, 0.0, np.inf, 1.0)):
        a = np.full((len(rows), ld), fill)
        for k, r in enumerate(rows):
            a[k, :len(r[i])] = r[i]
        out.append(a)
    return out


def betas(ladder=LADDER, cell=CELL):
    from transcriptioncycleinference_amd.mcmc import temper_ladder

    b = np.ones(len(ladder))
    for _, ch in TO.rungs(ladder).items():
        b[ch] = temper_ladder(7 + N_POINTS[cell[ch[0]]], len(ch))
    return b


def options(n_steps, **kw):
    from transcriptioncycleinference_amd.mcmc import DramOptions

    return DramOptions(**{**dict(n_steps=n_steps, burnintime=40, adaptint=AI, stats_from=1, thin=1, seed=11), **kw})


def run(lk, inp, o, cell=CELL, s20=1.0, **kw):
    from transcriptioncycleinference_amd.mcmc import dram_run

    return dram_run(lk, cell, *inp, s20, o, **kw)


def same_run(a, b, rows=slice(None)):
    np.testing.assert_array_equal(a.chain[:, rows], b.chain)
    np.testing.assert_array_equal(a.s2chain[:, rows], b.s2chain)
    np.testing.assert_array_equal(a.final_theta[rows], b.final_theta)
    np.testing.assert_array_equal(a.accept_rate[rows], b.accept_rate)
    np.testing.assert_array_equal(a.n_evals[rows], b.n_evals)


@pytest.mark.parametrize("n_steps, swap_every", [(101, 0), (15, 1)])
def test_beta_one_is_the_plain_sampler_bitwise(lk, small, n_steps, swap_every):
    inp = setup(small, CELL)
    o = options(n_steps)
    plain = run(lk, inp, o)
    t = run(lk, inp, o, beta=np.ones(len(CELL)), ladder=np.full(len(CELL), -1) if swap_every else None,
            swap_every=swap_every)
    same_run(t, plain)
    assert t.temper.n_events == 0 and not t.temper.swap_tried.any()


def test_fixed_sigma2_rung_is_a_plain_chain_at_sigma2_over_beta(lk, small):
    inp = setup(small, CELL)
    o = options(101, updatesigma=False)
    b = betas()
    t = run(lk, inp, o, s20=1.3, beta=b, ladder=LADDER, swap_every=0)
    plain = run(lk, inp, o, s20=1.3 / b)
    same_run(t, plain)
    assert np.all(t.s2chain == (1.3 / b)[None, :])


@pytest.fixture(scope="module")
def swapped(lk, small):
    """The swapped run of every engine: n_steps = 101, five swap events."""
    inp = setup(small, CELL)
    out = {e: run(lk, inp, options(101, engine=e), beta=betas(), ladder=LADDER, swap_every=1)
           for e in ("fused", "batched", "walk")}
    return inp, out


def test_engines_agree_on_a_swapped_run(swapped):
    _, runs = swapped
    a = runs["fused"]
    assert a.temper.n_events == 5 and a.temper.swap_tried.sum() > 0
    for e in ("batched", "walk"):
        b = runs[e]
        same_run(a, b)
        np.testing.assert_array_equal(a.temper.swap_logr, b.temper.swap_logr)   # NaN where no pair was tried
        np.testing.assert_array_equal(a.temper.swap_acc, b.temper.swap_acc)
        np.testing.assert_array_equal(a.temper.swap_tried, b.temper.swap_tried)
        np.testing.assert_array_equal(a.temper.swap_accepted, b.temper.swap_accepted)


def test_untouched_chain_in_a_tempered_call_has_the_plain_bits(lk, swapped):
    inp, runs = swapped
    one = [a[PLAIN:PLAIN + 1] for a in inp]
    plain = run(lk, one, options(101), cell=CELL[PLAIN:PLAIN + 1], chain_keys=np.array([PLAIN]))
    ld1 = plain.chain.shape[2]
    t = runs["fused"]
    np.testing.assert_array_equal(t.chain[:, PLAIN:PLAIN + 1, :ld1], plain.chain)
    np.testing.assert_array_equal(t.s2chain[:, PLAIN:PLAIN + 1], plain.s2chain)


@pytest.mark.parametrize("n_steps, n_events", [(15, 0), (100, 4), (101, 5)])
def test_swap_rule_follows_the_restatement(lk, small, n_steps, n_events):
    """swap_logr within the bound of the float64 restatement, swap_acc = (u < exp(logr)) wherever that is decidable,
    the pairs by parity, the counters the logs' column sums; at most 10 % of the events undecidable."""
    b = betas()
    nobs = 2.0 * np.array(N_POINTS)[CELL]
    events = undecided = 0
    for seed in (11, 12, 13):
        inp = setup(small, CELL, seed)
        o = options(n_steps, seed=seed)
        t = run(lk, inp, o, beta=b, ladder=LADDER, swap_every=1)
        tr = t.temper
        rows = TO.event_rows(n_steps, AI, 1)
        assert tr.n_events == n_events == len(rows) and tr.swap_logr.shape == (n_events, len(CELL))
        np.testing.assert_array_equal(tr.event_rows, rows)
        np.testing.assert_array_equal(tr.swap_tried, np.isfinite(tr.swap_logr).sum(axis=0))
        np.testing.assert_array_equal(tr.swap_accepted, tr.swap_acc.sum(axis=0))
        for e, s in enumerate(rows):
            assert s < n_steps
            pairs = TO.pairs_tried(LADDER, s, AI, 1)
            tried = np.zeros(len(CELL), bool)
            tried[[a for a, _ in pairs]] = True
            np.testing.assert_array_equal(~np.isnan(tr.swap_logr[e]), tried)   # the parity rule
            assert not tr.swap_acc[e][~tried].any()
            ss = lk.ss_batch(t.chain[s - 1], CELL)
            for a, c in pairs:
                lr, bound = TO.logr(b[a], b[c], ss[a], t.s2chain[s - 1, a], ss[c], t.s2chain[s - 1, c], nobs[a])
                print(f"seed {seed} row {s} pair ({a},{c}): logr {tr.swap_logr[e, a]!r} restated {lr!r} bound {bound:.3e}")
                assert abs(tr.swap_logr[e, a] - lr) <= bound
                u = TO.uniform_at(o.seed, a, s)
                events += 1
                if abs(lr - np.log(u)) > bound:
                    assert bool(tr.swap_acc[e, a]) == TO.accept(lr, u)
                else:
                    undecided += 1
    assert undecided <= 0.1 * events
    assert (events > 0) == (n_events > 0)


def test_accepted_swap_exchanges_the_two_states_exactly(lk, small):
    """With proposals that mostly leave the bounds the step after an event is rejected, so chain row s + 1 shows what
    the swap left: the other rung's row s when swap_acc is set, the rung's own otherwise. sigma2 is a constant here
    (updatesigma = 0) and never moves."""
    inp = setup(small, CELL, 3)
    inp[5] = inp[5] * 1e4    # qcov_diag
    b = betas()
    # burnintime = 0: no burn-in shrinking of the proposal, which would bring it back inside the bounds
    t = run(lk, inp, options(101, updatesigma=False, seed=5, burnintime=0), s20=1.1, beta=b, ladder=LADDER, swap_every=1)
    tr = t.temper
    checked = {True: 0, False: 0}
    for e, s in enumerate(tr.event_rows):
        for a, c in TO.pairs_tried(LADDER, s, AI, 1):
            before = {a: t.chain[s - 1, a], c: t.chain[s - 1, c]}
            acc = bool(tr.swap_acc[e, a])
            for x, y in ((a, c), (c, a)):
                after = t.chain[s, x]
                if not (np.array_equal(after, before[a]) or np.array_equal(after, before[c])):
                    continue   # the step moved the chain: nothing to read off this row
                np.testing.assert_array_equal(after, before[y] if acc else before[x])
                checked[acc] += 1
    assert checked[True] >= 1 and checked[False] >= 1, checked
    np.testing.assert_array_equal(t.s2chain, np.broadcast_to(1.1 / b, t.s2chain.shape))


def test_tempered_gibbs_draw_has_its_gamma_law(lk, small):
    """theta frozen (lower = upper = x0: every proposal is out of bounds), so 1 / s2t is iid Gamma(k = beta N / 2,
    scale 2 / ss0): its sample mean within 5 sqrt(k th^2 / n) of k th, its variance within 5 sqrt((2 k^2 + 6 k) th^4 / n)
    of k th^2."""
    cell = np.array([0, 0, 1, 1], np.int32)
    b = np.array([1.0, 0.5, 1.0, 0.5])
    inp = setup(small, cell, 7)
    inp[1], inp[2] = inp[0].copy(), inp[0].copy()
    n_rows = 20000
    t = run(lk, inp, options(n_rows, burnintime=0), cell=cell, beta=b, swap_every=0)
    assert np.all(t.n_evals == 1)
    ss0 = lk.ss_batch(inp[0], cell)
    x = 1.0 / t.s2chain[1:]   # row 1 is sigma2_0
    n = x.shape[0]
    for c in range(len(cell)):
        k, th = b[c] * N_POINTS[cell[c]], 2.0 / ss0[c]    # beta * N / 2 with N = 2 N_c
        m, v = x[:, c].mean(), x[:, c].var(ddof=1)
        print(f"chain {c}: mean {m!r} want {k * th!r} +- {5 * np.sqrt(k * th * th / n):.3e}; "
              f"var {v!r} want {k * th * th!r} +- {5 * np.sqrt((2 * k * k + 6 * k) * th ** 4 / n):.3e}")
        assert abs(m - k * th) <= 5 * np.sqrt(k * th * th / n)
        assert abs(v - k * th * th) <= 5 * np.sqrt((2 * k * k + 6 * k) * th ** 4 / n)


def test_cold_rung_samples_the_posterior_of_a_plain_chain(lk, small):
    """One 12-point cell with bounds drawn tight around a plain run's mean (a unimodal target): the cold rungs of four
    4-rung ladders against four plain chains, 20,000 steps each; every parameter's pooled mean within
    5 sqrt(mcse_1^2 + mcse_2^2), the MCSE from chainess on each run."""
    from transcriptioncycleinference_amd.mcmc import temper_ladder

    M, R, P = 4, 4, 7 + N_POINTS[0]
    pilot_in = setup(small, np.zeros(1, np.int32), 1)
    pilot = run(lk, pilot_in, options(4000, burnintime=2000, stats_from=2001, thin=0), cell=np.zeros(1, np.int32))
    lo0, hi0 = pilot_in[1][0], pilot_in[2][0]
    half = 0.02 * (hi0 - lo0)
    lo = np.maximum(lo0, pilot.mean[0] - half)
    hi = np.minimum(hi0, pilot.mean[0] + half)
    cell = np.zeros(M * R, np.int32)
    inp = setup(small, cell, 2)
    rng = np.random.default_rng(4)
    inp[0] = lo + (hi - lo) * rng.uniform(0.25, 0.75, (M * R, P))
    inp[1], inp[2] = np.tile(lo, (M * R, 1)), np.tile(hi, (M * R, 1))
    ladder = np.tile(np.arange(M, dtype=np.int32), R)            # chain q * M + r: rung q of ladder r
    b = np.repeat(temper_ladder(P, R), M)
    n_steps, burn = 20000, 5000
    o = options(n_steps, burnintime=burn, stats_from=burn + 1, thin=1, seed=21)
    t = run(lk, inp, o, cell=cell, beta=b, ladder=ladder, swap_every=1)
    plain = run(lk, [a[:M] for a in inp], dataclasses.replace(o, seed=22), cell=cell[:M])
    assert t.temper.swap_accepted.sum() > 0
    grp = np.zeros(M, np.int32)
    ce_t = lk.chainess(t.chain[burn:, :M], t.s2chain[burn:, :M], group=grp)
    ce_p = lk.chainess(plain.chain[burn:], plain.s2chain[burn:], group=grp)
    mt, mp = t.chain[burn:, :M].mean(axis=(0, 1)), plain.chain[burn:].mean(axis=(0, 1))
    tol = 5 * np.sqrt(ce_t.mcse[0, :P] ** 2 + ce_p.mcse[0, :P] ** 2)
    print("cold - plain:", mt - mp, "tolerance:", tol, "swap rate:",
          t.temper.swap_accepted.sum() / max(t.temper.swap_tried.sum(), 1))
    assert np.all(np.isfinite(tol))
    assert np.all(np.abs(mt - mp) <= tol)


def raw_call(lk, inp, o, cell, beta, ladder, n_ladders, swap_every, flags, s20=1.0):
    """tci_dram_run_tempered through ctypes with the context of `lk`: (status, message). What the Python wrapper never
    passes (flags != 0, a negative swap_every, an n_ladders that does not cover the ids) reaches the library here."""
    import ctypes as C

    from transcriptioncycleinference_amd import _lib

    f = lambda a: np.ascontiguousarray(a, np.float64)  # noqa: E731
    x = [f(a) for a in inp]
    n, ld = x[0].shape
    cid = np.ascontiguousarray(cell, np.int32)
    s2 = f(np.broadcast_to(np.asarray(s20, np.float64), (n,)))
    bt, ldr = f(beta), np.ascontiguousarray(ladder, np.int32)
    oc = o.to_c()
    out = _lib.tci_dram_outputs()
    topt = _lib.tci_temper_options(_lib.ptr(bt, _lib._dp), _lib.ptr(ldr, _lib._i32p), n_ladders, swap_every, flags)
    tout = _lib.tci_temper_outputs()
    rc = lk._lib.tci_dram_run_tempered(lk._h, C.byref(oc), n, _lib.ptr(cid, _lib._i32p), *[_lib.ptr(a, _lib._dp) for a in x],
                                       _lib.ptr(s2, _lib._dp), ld, C.byref(out), None, None, 0, None, None,
                                       C.byref(topt), C.byref(tout))
    return rc, lk._lib.tci_last_error(lk._h).decode()


def test_validation_names_the_ladder(lk, small):
    """Every rule of include/tci.h is TCI_EINVAL with the ladder (and chain) it failed on in the message; the rules the
    Python wrapper answers itself or cannot break (swap_every, flags, n_ladders) through the C ABI directly."""
    from transcriptioncycleinference_amd._lib import TCI_EINVAL, TCI_OK, TciError

    inp = setup(small, CELL)
    o = options(15)
    b = betas()

    def refused(names, inp=inp, o=o, s20=1.0, **kw):
        with pytest.raises(TciError) as ei:
            run(lk, inp, o, s20=s20, **{**dict(beta=b, ladder=LADDER, swap_every=1), **kw})
        assert ei.value.code == TCI_EINVAL and names in str(ei.value), (names, str(ei.value))

    for bad in (0.0, -0.5, 1.5, np.nan, np.inf):
        bb = b.copy()
        bb[1] = bad
        refused("(chain 1, ladder 0)", beta=bb)
    bb = b.copy()
    bb[3] = bb[2]                      # not strictly decreasing along ladder 1
    refused("(ladder 1, chains 2 and 3)", beta=bb)
    bb = b.copy()
    bb[[6, 7]] = bb[[7, 6]]            # increasing
    refused("(ladder 2, chains 6 and 7)", beta=bb)
    cell = CELL.copy()
    cell[1] = 1                        # ladder 0 across two cells
    with pytest.raises(TciError) as ei:
        run(lk, inp, o, cell=cell, beta=b, ladder=LADDER)
    assert ei.value.code == TCI_EINVAL and "share the cell (ladder 0, chains 0 and 1)" in str(ei.value)
    for i in (1, 2, 3, 4):             # lower, upper, prior_mu, prior_sig differ inside ladder 2
        x = [a.copy() for a in inp]
        x[i][7, 8] = {1: -29.0, 2: 29.0, 3: 0.5, 4: 40.0}[i]
        refused("(ladder 2, chains 6 and 7)", inp=x)
    refused("sigma2_0 (ladder 1, chains 2 and 3)", o=dataclasses.replace(o, updatesigma=False),
            s20=np.where(np.arange(len(CELL)) == 3, 2.0, 1.0))
    l = LADDER.copy()
    l[0] = -2
    refused("(chain 0, ladder -2)", ladder=l)
    small_beta = np.where(np.arange(len(CELL)) == PLAIN, 0.01, b)          # beta N / 2 < 1 on the chain in no ladder
    refused("(chain 5, ladder -1)", beta=small_beta)
    run(lk, inp, dataclasses.replace(o, updatesigma=False), beta=small_beta, ladder=LADDER)   # no Gibbs draw: no limit
    # through the ABI: the well-formed call passes, then one rule at a time
    nl = int(LADDER.max()) + 1
    assert raw_call(lk, inp, o, CELL, b, LADDER, nl, 1, 0)[0] == TCI_OK
    rc, msg = raw_call(lk, inp, o, CELL, b, LADDER, nl, -1, 0)
    assert rc == TCI_EINVAL and "swap_every must be >= 0" in msg
    rc, msg = raw_call(lk, inp, o, CELL, b, LADDER, nl, 1, 1)
    assert rc == TCI_EINVAL and "flags" in msg
    rc, msg = raw_call(lk, inp, o, CELL, b, LADDER, nl - 1, 1, 0)          # ladder 2 is outside [-1, 2)
    assert rc == TCI_EINVAL and "[-1, n_ladders)" in msg and "(chain 6, ladder 2)" in msg
    for bad_n in (-1, len(CELL) + 1):
        rc, msg = raw_call(lk, inp, o, CELL, b, LADDER, bad_n, 1, 0)
        assert rc == TCI_EINVAL and "n_ladders" in msg
    assert raw_call(lk, inp, o, CELL, b, LADDER, nl, 0, 0)[0] == TCI_OK     # 0: never swap


def test_tempered_call_carries_the_reductions(lk, small):
    """stats, cov, quant, dens and group through tci_dram_run_tempered: with every beta 1 and no swaps, the bits of the
    plain run's reductions."""
    inp = setup(small, CELL)
    o = options(101, stats_from=41)
    kw = dict(stats=True, cov=True, quant=(0.1, 0.5), dens=dict(n_grid=16, n_bins=8), group=CELL)
    plain = run(lk, inp, o, **kw)
    t = run(lk, inp, o, beta=np.ones(len(CELL)), swap_every=0, **kw)
    same_run(t, plain)
    for part, fields in (("stats", ("tau", "mcerr", "geweke_p")), ("cov", ("mean", "cov", "corr")), ("quant", ("q", "s2_q")),
                         ("dens", ("dens", "counts")), ("rhat", ("rhat", "rhat_split", "pooled_mean"))):
        assert getattr(getattr(t, part), "n_rows") == getattr(getattr(plain, part), "n_rows") > 0
        for f in fields:
            np.testing.assert_array_equal(getattr(getattr(t, part), f), getattr(getattr(plain, part), f), err_msg=f)


def test_fit_with_a_ladder_end_to_end(lk, small):
    """fit(temper=R): temper = 1 is the untempered fit bit for bit; temper = 2 runs the layout of temper_layout, keeps
    every existing field the cold rungs' (those of the same dram_run call, sliced) and fills MCMCtemper, with ess and
    logpost reduced from the cold rungs' kept rows."""
    from transcriptioncycleinference_amd.mcmc import (DramOptions, dram_run, fit, plan_fit, replicate_keys, temper_ladder,
                                                        temper_layout)

    kw = dict(n_steps=201, n_burn=81, seed=3, thin=2, replicates=2, opts=DramOptions(adaptint=AI))
    base = fit(lk, **kw)
    one = fit(lk, temper=1, **kw)
    assert one.MCMCtemper is None
    for a, c in zip(one.MCMCresults + one.MCMCchain, base.MCMCresults + base.MCMCchain):
        for f in a:
            np.testing.assert_array_equal(a[f], c[f], err_msg=f)
    np.testing.assert_array_equal(one.MCMCrhat[0]["rhat"], base.MCMCrhat[0]["rhat"])
    M, R, K = 2, 2, 2
    fr = fit(lk, temper=R, ess=True, logpost=True, **kw)
    # the same call by hand
    plan = plan_fit(small, [0, 1], 3, replicates=M * R)
    o = DramOptions(n_steps=201, burnintime=81, stats_from=81, thin=2, adaptint=AI, seed=3 * 1000003 + 20201028)
    lay = temper_layout(list(N_POINTS), M, R)
    res = dram_run(lk, np.tile(np.array([0, 1], np.int32), M * R), plan.x0, plan.lower, plan.upper, plan.prior_mu,
                   plan.prior_sig, plan.qcov_diag, 1.0, o, chain_keys=replicate_keys(np.arange(K), M * R), **lay)
    assert res.temper.n_events == 10 and res.temper.swap_tried.sum() > 0
    sel = 1 + 2 * np.arange(res.chain.shape[0]) >= 81
    for k in range(K):
        P = 7 + N_POINTS[k]
        assert fr.MCMCresults[k]["mean_v"] == res.mean[k, 0] and fr.MCMCresults[k]["mean_sigma"] == res.sigma_mean[k]
        np.testing.assert_array_equal(fr.MCMCresults[k]["mean_dR"], res.mean[k, 7:P])
        np.testing.assert_array_equal(fr.MCMCchain[k]["dR_chain"], res.chain[sel, k, 7:P])
        np.testing.assert_array_equal(fr.MCMCchain[k]["s2chain"], res.s2chain[:, k])
        np.testing.assert_array_equal(fr.MCMCrhat[k]["mean_rep"], res.mean[[k, K + k], :P])      # the cold rungs only
        np.testing.assert_array_equal(fr.MCMCrhat[k]["accept_rep"], res.accept_rate[[k, K + k]])
        e = fr.MCMCtemper[k]
        np.testing.assert_array_equal(e["beta"], temper_ladder(P, R))
        rungs = np.array([[k, M * K + k], [K + k, M * K + K + k]])                                   # [replicate, rung]
        np.testing.assert_array_equal(e["accept_rate"], res.accept_rate[rungs])
        np.testing.assert_array_equal(e["swap_tried"][:, 0], res.temper.swap_tried[rungs[:, 0]])
        assert e["n_events"] == 10 and e["n_chains"] == M * R
        assert fr.MCMCess[k]["n_chains"] == M and np.all(np.isfinite(fr.MCMCess[k]["ess"][:P]))
        assert fr.MCMClp[k]["ss"].shape == (M, int(sel.sum())) and np.isfinite(fr.MCMClp[k]["ss_gap"])
        ss = lk.ss_batch(res.chain[sel][:, K + k], np.full(int(sel.sum()), k, np.int32))          # replicate 1, cold
        np.testing.assert_array_equal(fr.MCMClp[k]["ss"][1], ss)
    np.testing.assert_array_equal(fr.accept_rate, res.accept_rate[:K])
    np.testing.assert_array_equal(fr.final_theta, res.final_theta[:K])
    assert fr.n_evals == int(res.n_evals.sum())
