"""The replica exchange (k_swap, tci_dram.hip) on rows longer than a wavefront and in calls of many ladders, which
tests/test_temper_gpu.py (cells of 12 and 17 points, at most 6 pairs) leaves out. k_swap exchanges two rows with
`for (j = lane; j < P; j += 64)`: at P = 72, 137 and 264 the loop takes 2, 3 and 5 trips, and with ld = 264 the shorter
rows have padding the exchange must leave alone. The methods are that module's.

Layout (tests/ragged_cases.py's "rpl4" context, rows_per_lane 4): on each of the 65-, 130- and 257-point cells eight
2-rung and four 3-rung ladders; a 9-rung ladder on the 130-point cell, a 6-rung ladder on the 257-point cell, a 2-rung
ladder on the 2-point cell (its beta N / 2 >= 1 admits no third rung) and one 257-point chain in no ladder: 102 chains,
62 pairs, 16 workgroups of k_swap. The chains are dealt so that no two rungs of a ladder are neighbours. adaptint = 20,
swap_every = 1, n_steps = 101: five swap events."""
import numpy as np
import pytest

import ragged_cases as RC
import temper_oracle as TO
from test_temper_gpu import AI, options, run, same_run, setup

pytestmark = pytest.mark.gpu

LONG = (65, 130, 257)
AT = RC.primary_cells("rpl4")
LD = 264
PAD = 7.0     # chain i's theta0 holds PAD + i past its P


def deal():
    """(points, ladder id, rung) per chain. The next chain is the next rung of the ladder with the most rungs left
    among those that did not give the previous chain, so rungs of one ladder never sit side by side."""
    ladders = []
    for n in LONG:
        ladders += [(n, 2)] * 8 + [(n, 3)] * 4
    ladders += [(130, 9), (257, 6), (2, 2), (257, 1)]    # the last one: the chain in no ladder
    left = [r for _, r in ladders]
    out, last = [], -1
    while sum(left):
        l = max((q for q in range(len(ladders)) if left[q] and q != last), key=lambda q: (left[q], -q))
        n, r = ladders[l]
        out.append((n, l if r > 1 else -1, r - left[l]))
        left[l] -= 1
        last = l
    return tuple(np.array(a) for a in zip(*out))


NPTS, LADDER, RUNG = deal()
LADDER = LADDER.astype(np.int32)
CELL = np.array([AT[int(n)] for n in NPTS], np.int32)
NPAR = 7 + NPTS
PLAIN = int(np.nonzero(LADDER < 0)[0][0])
N_PAIRS = sum(len(ch) - 1 for ch in TO.rungs(LADDER).values())


def betas():
    from transcriptioncycleinference_amd.mcmc import temper_ladder

    return np.array([temper_ladder(int(p), 9)[r] for p, r in zip(NPAR, RUNG)])


@pytest.fixture(scope="module")
def lk():
    from transcriptioncycleinference_amd import Likelihood, from_lists

    with Likelihood(from_lists(RC.context_cells("rpl4")[0], "rpl4"), "P2P-MS2v5-LacZ-PP7v4", device=0) as L:
        assert L.info["rows_per_lane"] == 4 and all(int(L.cells.lengths[c]) == n for n, c in AT.items())
        yield L


def inputs(lk, seed):
    """test_temper_gpu.setup's rows for this layout, with PAD + i in the padding of chain i's theta0."""
    inp = setup(lk.cells, CELL, seed)
    assert inp[0].shape == (len(CELL), LD)
    for i, p in enumerate(NPAR):
        inp[0][i, p:] = PAD + i
    return inp


def test_the_layout_is_the_one_described():
    assert len(CELL) == 102 and N_PAIRS == 62 and (N_PAIRS + 3) // 4 == 16     # k_swap: four pairs per workgroup
    per = {n: sorted(len(ch) for ch in TO.rungs(LADDER).values() if NPTS[ch[0]] == n) for n in (2,) + LONG}
    assert per == {2: [2], 65: [2] * 8 + [3] * 4, 130: [2] * 8 + [3] * 4 + [9], 257: [2] * 8 + [3] * 4 + [6]}
    assert np.sum(LADDER < 0) == 1 and NPTS[PLAIN] == 257
    b = betas()
    for ch in TO.rungs(LADDER).values():
        assert np.all(np.diff(ch) > 1)                                        # no two rungs are neighbours
        assert len(set(CELL[ch])) == 1 and np.all(np.diff(b[ch]) < 0) and b[ch[0]] == 1.0
        assert np.all(RUNG[ch] == np.arange(len(ch)))


@pytest.fixture(scope="module")
def swapped(lk):
    """The swapped run of every engine, sigma2 updated: n_steps = 101, five swap events."""
    inp = inputs(lk, 11)
    out = {e: run(lk, inp, options(101, engine=e), cell=CELL, beta=betas(), ladder=LADDER, swap_every=1)
           for e in ("fused", "batched", "walk")}
    return inp, out


def test_swap_rule_follows_the_restatement_on_long_rows(lk, swapped):
    """test_temper_gpu.test_swap_rule_follows_the_restatement on this layout. The restated logr of an event comes from
    ss_batch of the chain row the event follows, so an exchange that moved ss without all of theta shows at the next
    event that tries a chain of the swapped pair; such events are counted per cell length."""
    _, runs = swapped
    t = runs["fused"]
    tr, b, o = t.temper, betas(), options(101)
    nobs = 2.0 * NPTS
    rows = TO.event_rows(101, AI, 1)
    assert tr.n_events == 5 == len(rows) and tr.swap_logr.shape == (5, len(CELL))
    np.testing.assert_array_equal(tr.event_rows, rows)
    np.testing.assert_array_equal(tr.swap_tried, np.isfinite(tr.swap_logr).sum(axis=0))
    np.testing.assert_array_equal(tr.swap_accepted, tr.swap_acc.sum(axis=0))
    events = undecided = 0
    ladder_swapped, chain_swapped = set(), set()
    after_ladder, after_chain = {n: 0 for n in LONG}, {n: 0 for n in LONG}
    for e, s in enumerate(rows):
        pairs = TO.pairs_tried(LADDER, s, AI, 1)
        tried = np.zeros(len(CELL), bool)
        tried[[a for a, _ in pairs]] = True
        np.testing.assert_array_equal(~np.isnan(tr.swap_logr[e]), tried)   # the parity rule
        assert not tr.swap_acc[e][~tried].any()
        ss = lk.ss_batch(t.chain[s - 1], CELL)
        for a, c in pairs:
            lr, bound = TO.logr(b[a], b[c], ss[a], t.s2chain[s - 1, a], ss[c], t.s2chain[s - 1, c], nobs[a])
            assert abs(tr.swap_logr[e, a] - lr) <= bound, (s, a, c, tr.swap_logr[e, a], lr, bound)
            u = TO.uniform_at(o.seed, a, s)
            events += 1
            if abs(lr - np.log(u)) > bound:
                assert bool(tr.swap_acc[e, a]) == TO.accept(lr, u)
            else:
                undecided += 1
            n = int(NPTS[a])
            if n in after_ladder:
                after_ladder[n] += LADDER[a] in ladder_swapped
                after_chain[n] += a in chain_swapped or c in chain_swapped
        for a, c in pairs:
            if tr.swap_acc[e, a]:
                ladder_swapped.add(LADDER[a])
                chain_swapped.update((a, c))
    print(f"{events} pair events, {int(tr.swap_accepted.sum())} accepted, {undecided} undecidable "
          f"({100.0 * undecided / events:.1f} %, cap 10 %)")
    print(f"pairs tried after an accepted swap of their ladder, per cell length: {after_ladder}; "
          f"of one of their own two chains: {after_chain}")
    assert undecided <= 0.1 * events
    assert all(v >= 1 for v in after_ladder.values()), after_ladder


def test_engines_agree_on_a_swapped_run_of_long_rows(swapped):
    _, runs = swapped
    a = runs["fused"]
    assert a.temper.n_events == 5 and a.temper.swap_accepted.sum() > 0
    for e in ("batched", "walk"):
        b = runs[e]
        same_run(a, b)
        np.testing.assert_array_equal(a.temper.swap_logr, b.temper.swap_logr)   # NaN where no pair was tried
        np.testing.assert_array_equal(a.temper.swap_acc, b.temper.swap_acc)
        np.testing.assert_array_equal(a.temper.swap_tried, b.temper.swap_tried)
        np.testing.assert_array_equal(a.temper.swap_accepted, b.temper.swap_accepted)


def test_the_chain_in_no_ladder_has_the_plain_bits(lk, swapped):
    inp, runs = swapped
    one = [a[PLAIN:PLAIN + 1] for a in inp]
    plain = run(lk, one, options(101), cell=CELL[PLAIN:PLAIN + 1], chain_keys=np.array([PLAIN]))
    assert plain.chain.shape[2] == LD
    t = runs["fused"]
    np.testing.assert_array_equal(t.chain[:, PLAIN:PLAIN + 1], plain.chain)
    np.testing.assert_array_equal(t.s2chain[:, PLAIN:PLAIN + 1], plain.s2chain)
    np.testing.assert_array_equal(t.final_theta[PLAIN:PLAIN + 1], plain.final_theta)


def test_padding_is_left_alone(swapped):
    """What lies past a chain's P. The sampler's state keeps theta0's padding, which final_theta returns (include/tci.h),
    here PAD + i: an exchange that ran past P would leave another chain's value there. The kept chain rows are 0 past P
    (include/tci.h), in every row of the run."""
    _, runs = swapped
    for e, t in runs.items():
        assert t.temper.swap_accepted.sum() > 0
        for i, p in enumerate(NPAR):
            assert np.all(t.final_theta[i, p:] == PAD + i), (e, i)
            assert np.all(t.chain[:, i, p:] == 0.0), (e, i)


def test_accepted_swap_exchanges_whole_rows(lk):
    """test_temper_gpu.test_accepted_swap_exchanges_the_two_states_exactly on this layout: with proposals that mostly
    leave the bounds the step after an event is rejected, so chain row s + 1 shows what the swap left: the other rung's
    whole row s when swap_acc is set, the rung's own otherwise. Both outcomes must be seen at every long cell length
    (12 ladders each; measured: 14 | 17, 21 | 22 and 11 | 29 rows read off after an accepted | a rejected swap). The
    one 2-rung ladder of the 2-point cell is tried twice only, and in the measured run the step after either event
    moved its chains, so no row of it was read off; it is in the layout for its 255 columns of padding beside the long
    rows, and a row of 9 parameters is the one-trip exchange tests/test_temper_gpu.py already holds."""
    inp = inputs(lk, 3)
    inp[5] = inp[5] * 1e4    # qcov_diag
    b = betas()
    t = run(lk, inp, options(101, updatesigma=False, seed=5, burnintime=0), cell=CELL, s20=1.1, beta=b, ladder=LADDER,
            swap_every=1)
    tr = t.temper
    assert t.chain.shape[2] == LD
    checked = {int(n): {True: 0, False: 0} for n in (2,) + LONG}
    for e, s in enumerate(tr.event_rows):
        for a, c in TO.pairs_tried(LADDER, s, AI, 1):
            before = {a: t.chain[s - 1, a], c: t.chain[s - 1, c]}
            acc = bool(tr.swap_acc[e, a])
            for x, y in ((a, c), (c, a)):
                after = t.chain[s, x]
                if not (np.array_equal(after, before[a]) or np.array_equal(after, before[c])):
                    continue   # the step moved the chain: nothing to read off this row
                np.testing.assert_array_equal(after, before[y] if acc else before[x])
                checked[int(NPTS[a])][acc] += 1
    print(f"rows read off after an event, per cell length {{accepted: n, rejected: n}}: {checked}")
    for n in LONG:
        assert checked[n][True] >= 1 and checked[n][False] >= 1, checked
    np.testing.assert_array_equal(t.s2chain, np.broadcast_to(1.1 / b, t.s2chain.shape))
    for i, p in enumerate(NPAR):
        assert np.all(t.final_theta[i, p:] == PAD + i) and np.all(t.chain[:, i, p:] == 0.0), i


def test_fit_reduces_the_log_posterior_of_swapped_137_parameter_chains(lk):
    """fit(temper=2, logpost=True) on the 130-point cell, two replicates: MCMClp's ss is ss_batch of the cold rungs' kept
    rows, as test_temper_gpu.test_fit_with_a_ladder_end_to_end holds it at P = 19. The same call by hand gives the rows."""
    from transcriptioncycleinference_amd.mcmc import (DramOptions, chain_theta, dram_run, fit, plan_fit, replicate_keys,
                                                        temper_layout)

    c, M, R = AT[130], 2, 2
    fr = fit(lk, cells=[c], n_steps=201, n_burn=81, seed=3, thin=2, replicates=M, temper=R, logpost=True,
             opts=DramOptions(adaptint=AI))
    plan = plan_fit(lk.cells, [c], 3, replicates=M * R)
    o = DramOptions(n_steps=201, burnintime=81, stats_from=81, thin=2, adaptint=AI, seed=3 * 1000003 + 20201028)
    res = dram_run(lk, np.full(M * R, c, np.int32), plan.x0, plan.lower, plan.upper, plan.prior_mu, plan.prior_sig,
                   plan.qcov_diag, 1.0, o, chain_keys=replicate_keys(np.array([c]), M * R), **temper_layout([130], M, R))
    print(f"swaps tried {res.temper.swap_tried[:M].tolist()}, accepted {res.temper.swap_accepted[:M].tolist()}")
    assert res.temper.n_events == 10 and res.temper.swap_accepted.sum() > 0
    sel = 1 + 2 * np.arange(res.chain.shape[0]) >= 81
    kept = res.chain[sel]
    np.testing.assert_array_equal(chain_theta(fr.MCMCchain[0], 130, np.arange(int(sel.sum()))), kept[:, 0, :137])
    assert fr.MCMClp[0]["ss"].shape == (M, int(sel.sum()))
    for r in range(M):
        np.testing.assert_array_equal(fr.MCMClp[0]["ss"][r], lk.ss_batch(kept[:, r], np.full(len(kept), c, np.int32)))
