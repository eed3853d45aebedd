"""The DE-MC(zs) kernels (k_zs_propose / k_zs_decide, tci_demczs.hip) and their host loop (tci_api_demczs.cpp) at the
shapes tests/test_demczs_gpu.py leaves out. The method is that module's: the numpy restatement (tests/demczs_oracle.py)
with Likelihood.ss_batch as its SS function, the device's ljac held to the restatement's own within ljac_bound and then
forced, every other output, the archive included, compared bit for bit, every decision decidable.

  rows         P = 2055 (the 2,048-point cell of ragged_cases' "tile_max": 33 trips of every lane loop, 33 bits of the
               crossing mask, h = 1027 in ljac), P = 9 beside it at ld = 2055, every cell of "rpl4" (2 to 257 points)
               and of a context built here whose cells of 2, 57, 58, 121 and 122 points give P = 9, 64, 65, 128, 129: the
               last trip of every lane loop is full or holds lane 0 alone. The padding of pop0 and of z0 carries two
               different marks: a chain's padding is its parent's, an archive row's is z0's below m0 and the chain's
               above. Three chains per cell make B no multiple of k_zs_propose's four waves.
  populations  1,024 to 4,096 chains on P = 9 with m0 = 3: the second index call's counter up to 8,191, the Gamma stream
               base i << 16 up to 2^28 - 2^16, sh_take full, 4,096 rows appended by one launch and read by the next
               generation, null moves of the chains the archive starts from.
  archive      m0 = 2^16 + 5 rows, so that m(w, M) gives indices at and above 2^16: the rows are drawn with
               numpy.random.default_rng around the chains' starts, within ARCHIVE_FRACTION of [lower, upper] on either
               side and clipped into the box. The fraction is an input, not a tolerance: at 0.05 the 16 decisions of the
               run hold accepts of both move types, rejects and out-of-bounds trials, at least two of each (from 0.1 on
               the restatement accepts no snooker move, at 0.002 it rejects two trials). ARCHIVE_KEY is the first RNG stream key
               on which a chain of generation 3 or 4 reads one of the four rows appended after generation 2, a row
               index at or above m0 > 2^16. An archive near the 2^24-row cap needs more than 1 GB on the device and as
               much again on the host, so only its refusal stays tested (tests/test_demczs_gpu.py).
  logs, kept   log_rows below, at and above n_gen and 0; thin = 0 (the device holds no chain) and thin > n_gen; a run
               whose generations keep only, append only, do both and do neither.

Every group's runs must accept, reject and leave the box (and meet null moves where m0 < n_pop): a run in which nothing
moves would replay trivially. The jitter is 40 times the default, as in tests/test_demczs_gpu.py."""
import dataclasses

import numpy as np
import pytest

import demczs_oracle as O
import ragged_cases as RC
import variant_rows as VR
from test_demc_shapes_gpu import PAD, marked_padding, rpl4, tile_max  # noqa: F401  (the two context fixtures)
from test_demczs_gpu import (KEPT, LOGS, MEMBER, S2_RTOL, SEED, Plan, assert_cell, assert_ljac, cell_view, device,
                             oracle_cell)

pytestmark = pytest.mark.gpu

ZPAD = 9.0                   # written into z0's padding; PAD (7.0) into pop0's
FIELDS = KEPT + MEMBER + LOGS + ("archive",)
EDGE = (2, 57, 58, 121, 122)                 # points: P = 9, 64, 65, 128, 129
ROW_KW = dict(n_gen=3, jump_every=3, thin=1, append_every=1, log_rows=3, archive=True)   # generation 3 is a jump
ROW_M0 = 8
POPS = (1024, 1025, 4095, 4096)
POP_KW = dict(n_gen=2, jump_every=2, thin=1, append_every=1, CR=0.3, p_snooker=0.5, log_rows=2, archive=True)
ARCHIVE_M0 = 2 ** 16 + 5
ARCHIVE_FRACTION = 0.05
ARCHIVE_KEY = 249
ARCHIVE_KW = dict(n_gen=4, jump_every=3, thin=1, append_every=2, CR=0.3, p_snooker=0.5, log_rows=4, archive=True)
LOG_SHAPE = (70, 90)         # n_pop, m0


def edge_cells():
    rng = np.random.default_rng(9000 + sum(EDGE))
    return [VR.synthetic_cell_list(rng, n, n_cells=1)[0] for n in EDGE]


@pytest.fixture(scope="module")
def lane_edge():
    from transcriptioncycleinference_amd import Likelihood, from_lists

    with Likelihood(from_lists(edge_cells(), "lane_edge"), "P2P-MS2v5-LacZ-PP7v4", device=0) as L:
        assert L.info["rows_per_lane"] == 2      # 121 steps: past 64, within 128
        assert tuple(7 + int(n) for n in L.cells.lengths) == (9, 64, 65, 128, 129)
        yield L, {n: c for c, n in enumerate(EDGE)}


def plan(L, ids, n_pop, m0, scale=40.0, mark=False):
    """test_demczs_gpu.plan for the context L (not cached: that one's key does not hold the context). mark: PAD in
    pop0's entries past each cell's P and ZPAD in z0's."""
    from transcriptioncycleinference_amd import mcmc

    sp = mcmc.search_population(L.cells, ids, SEED, max(n_pop, m0))
    jit = np.zeros_like(sp.lower)
    base = mcmc.demc_jitter(L.cells, sp.cells)
    jit[:, :base.shape[1]] = scale * base
    pl = Plan(tuple(sp.cells), sp.pop0[:, :n_pop].copy(), sp.pop0[:, :m0].copy(), sp.lower, sp.upper, sp.prior_mu,
              sp.prior_sig, jit)
    if mark:
        pl = marked_padding(L, pl)
        z0 = pl.z0.copy()
        for k, c in enumerate(pl.cells):
            z0[k, :, 7 + int(L.cells.lengths[c]):] = ZPAD
        pl = dataclasses.replace(pl, z0=z0)
    return pl


def replayed(L, pl, got, k, n_pop, key=None, **kw):
    """Cell k of the device run got against the restatement under the same options; returns the restatement."""
    want = oracle_cell(L, pl, k, key=k if key is None else key, got=got, n_pop=n_pop, **kw)
    assert want["undecided"] == [], f"cell {k}: pick another SEED"
    assert_ljac(got, k, want, n_pop)
    assert_cell(got, k, want, n_pop)
    return want


def counts(runs):
    """(accepts, rejects, out of bounds, null moves, accepted snooker moves) over the device runs, after the structural
    relations of test_demczs_gpu.test_the_replayed_runs_move on each."""
    for g in runs:
        assert np.all(np.isnan(g.logr) == (g.trial_oob != 0)) and not np.any(g.accepted & (g.trial_oob != 0))
        assert np.all(g.snooker[g.trial_oob == 2] == 1) and np.all(g.ljac[g.snooker == 0] == 0)
        assert np.all(np.isnan(g.ljac) == ((g.snooker == 1) & (g.trial_oob != 0)))
        assert g.logr.shape[0] == g.n_gen      # every generation is in the logs, so the counters are their sums
        assert np.all(g.n_null.reshape(-1) == (g.trial_oob == 2).sum(axis=0))
        assert np.all(g.n_oob.reshape(-1) == (g.trial_oob == 1).sum(axis=0))
        np.testing.assert_array_equal(g.accept_rate.reshape(-1), g.accepted.sum(axis=0) / g.n_gen)
    return (sum(int(g.accepted.sum()) for g in runs), sum(int(((1 - g.accepted) & (g.trial_oob == 0)).sum()) for g in runs),
            sum(int((g.trial_oob == 1).sum()) for g in runs), sum(int((g.trial_oob == 2).sum()) for g in runs),
            sum(int((g.accepted & g.snooker).sum()) for g in runs))


def moves(name, runs, nulls):
    acc, rej, oob, null, snk_acc = counts(runs)
    n = sum(g.accepted.size for g in runs)
    print(f"{name}: {acc} accepts ({snk_acc} of snooker moves), {rej} rejects, {oob} out of bounds, {null} null moves "
          f"of {n} decisions")
    assert acc > 0 and rej > 0 and oob > 0 and snk_acc > 0
    assert null > 0 or not nulls


# ---------------------------------------------------------------------------------------------------------------------
# row lengths and padding

_row_runs = {}


def row_run(L, tag, ids, n_pop, p_snooker, CR, keys=None, mark=True):
    """(plan, device run) of the cells ids of the context tag in one call, computed once."""
    key = (tag, tuple(ids), n_pop, p_snooker, CR, keys)
    if key not in _row_runs:
        pl = plan(L, ids, n_pop, ROW_M0, mark=mark)
        _row_runs[key] = pl, device(L, pl, CR=CR, p_snooker=p_snooker, keys=None if keys is None else list(keys), **ROW_KW)
    return _row_runs[key]


def same_alone(L, tag, pl, got, k, n_pop, p_snooker, CR):
    """Cell k of the mixed call against a run of it alone at ld = P under the same key, in every field; its padding in
    the mixed call is its parents' in pop and chain, z0's in the archive rows below m0 and the chains' above."""
    c = pl.cells[k]
    P = 7 + int(L.cells.lengths[c])
    one, alone = row_run(L, tag, (c,), n_pop, p_snooker, CR, keys=(k,), mark=False)
    assert one.pop0.shape[2] == P < pl.pop0.shape[2]
    for f in FIELDS:
        a, b = cell_view(alone, f, 0, n_pop), cell_view(got, f, k, n_pop)
        if f in ("chain", "pop", "archive"):
            b = b[..., :P]
        np.testing.assert_array_equal(a, b, err_msg=f"{f} of cell {k}")
    assert np.all(got.pop[k, :, P:] == PAD) and np.all(cell_view(got, "chain", k, n_pop)[..., P:] == PAD)
    assert np.all(got.archive[k, :ROW_M0, P:] == ZPAD) and np.all(got.archive[k, ROW_M0:, P:] == PAD)


LONG = [(0.0, 0.0), (0.0, 1.0), (1.0, 0.3), (0.5, 0.3)]   # p_snooker, CR


@pytest.mark.parametrize("p_snooker,CR", LONG)
def test_2048_point_cell_replays_bit_for_bit(tile_max, p_snooker, CR):
    """P = 2055. Parallel moves with CR = 1 set all 33 bits of the crossing mask in lanes 0 to 6, with CR = 0 jrand's
    alone; snooker moves sum 33 terms per lane three times and scale their log ratio by h = 1027."""
    L, at = tile_max
    pl, got = row_run(L, "tile_max", (at[2048],), 5, p_snooker, CR)
    assert got.chain.shape == (4, 5, 2055) and got.archive.shape == (1, ROW_M0 + 15, 2055) and got.n_archive == ROW_M0 + 15
    replayed(L, pl, got, 0, 5, CR=CR, p_snooker=p_snooker, **ROW_KW)
    assert got.snooker.mean() == p_snooker if p_snooker in (0.0, 1.0) else 0 < got.snooker.mean() < 1
    if CR == 0.0 and p_snooker == 0.0:   # d' = 1: a chain that moved in generation 1 or 2 moved in jrand's coordinate alone
        for g in (1, 2):
            assert np.all(np.sum(got.chain[g] != got.chain[g - 1], axis=1) <= 1)
        assert np.any(got.chain[2] != got.chain[0])


def test_a_two_point_cell_beside_a_2048_point_cell(tile_max):
    L, at = tile_max
    pl, got = row_run(L, "tile_max", (at[2048], at[2]), 5, 0.5, 0.3)
    assert got.chain.shape == (4, 10, 2055)
    for k in range(2):
        replayed(L, pl, got, k, 5, CR=0.3, p_snooker=0.5, **ROW_KW)
    same_alone(L, "tile_max", pl, got, 1, 5, 0.5, 0.3)


@pytest.mark.parametrize("tag", ["lane_edge", "rpl4"])
def test_every_cell_of_a_context_in_one_call(request, tag):
    """Three chains per cell: B is no multiple of k_zs_propose's four waves, so its last block has idle waves and most
    blocks hold chains of two cells."""
    L, _ = request.getfixturevalue(tag)
    ids = tuple(range(L.cells.n_cells))
    assert len(ids) == (len(EDGE) if tag == "lane_edge" else len(RC.context_cells("rpl4")[0]))
    pl, got = row_run(L, tag, ids, 3, 0.5, 0.3)
    assert got.logr.shape == (3, 3 * len(ids)) and (3 * len(ids)) % 4 != 0
    ld = pl.pop0.shape[2]
    short = 0
    for k, c in enumerate(pl.cells):
        replayed(L, pl, got, k, 3, CR=0.3, p_snooker=0.5, **ROW_KW)
        if 7 + int(L.cells.lengths[c]) < ld:
            same_alone(L, tag, pl, got, k, 3, 0.5, 0.3)
            short += 1
    assert short == len(ids) - 1      # all but the longest cell


def test_the_row_length_runs_move(tile_max, lane_edge, rpl4):
    L, at = tile_max
    runs = [row_run(L, "tile_max", (at[2048],), 5, p, CR)[1] for p, CR in LONG]
    runs.append(row_run(L, "tile_max", (at[2048], at[2]), 5, 0.5, 0.3)[1])
    for tag, (L, _) in (("lane_edge", lane_edge), ("rpl4", rpl4)):
        runs.append(row_run(L, tag, tuple(range(L.cells.n_cells)), 3, 0.5, 0.3)[1])
    moves("row lengths", runs, nulls=False)     # m0 = 8 >= n_pop


# ---------------------------------------------------------------------------------------------------------------------
# populations

_pop_runs = {}


def pop_run(L, at, n_pop, updatesigma=False):
    """(plan, device run) of n_pop chains on the 2-point cell with m0 = 3: the archive starts as the first three chains'
    starts, and generation 2 reads 3 + n_pop rows, all but three appended by generation 1's one launch."""
    key = (n_pop, updatesigma)
    if key not in _pop_runs:
        pl = plan(L, (at[2],), n_pop, 3)
        _pop_runs[key] = pl, device(L, pl, updatesigma=updatesigma, **POP_KW)
    return _pop_runs[key]


@pytest.mark.parametrize("n_pop", POPS)
def test_full_populations_replay_bit_for_bit(rpl4, n_pop):
    L, at = rpl4
    pl, got = pop_run(L, at, n_pop)
    assert got.chain.shape == (3, n_pop, 9) and got.logr.shape == (2, n_pop)
    assert got.n_archive == 3 + 2 * n_pop == got.archive.shape[1]
    np.testing.assert_array_equal(pl.z0[0], pl.pop0[0, :3])
    replayed(L, pl, got, 0, n_pop, **POP_KW)
    assert np.all(got.n_evals == 3 - got.n_oob - got.n_null)
    np.testing.assert_array_equal(got.archive[0, 3:].reshape(2, n_pop, 9), got.chain[1:])
    assert 0.4 < got.snooker.mean() < 0.6


def test_gamma_streams_of_4096_chains(rpl4):
    """updatesigma = 1 with 4,096 chains: the restatement's decisions forced on the device's own s2chain, each of its s2
    draws (Philox and Marsaglia-Tsang restated in Python, stream base i << 16 up to 2^28 - 2^16) held to the device's
    within S2_RTOL, and no two chains sharing a stream."""
    L, at = rpl4
    n_pop = 4096
    pl, got = pop_run(L, at, n_pop, updatesigma=True)
    forced = cell_view(got, "s2chain", 0, n_pop)
    want = oracle_cell(L, pl, 0, key=0, got=got, n_pop=n_pop, updatesigma=True, forced_s2=forced, **POP_KW)
    assert want["undecided"] == [], "pick another SEED"
    np.testing.assert_array_equal(forced[0], np.ones(n_pop))
    np.testing.assert_allclose(forced[1:], want["s2_draw"], rtol=S2_RTOL, atol=0)
    assert_ljac(got, 0, want, n_pop)
    assert_cell(got, 0, want, n_pop, fields=("chain", "sschain", "prichain", "pop", "ss", "accept_rate", "n_oob", "n_null",
                                             "n_evals", "archive") + LOGS)
    np.testing.assert_array_equal(got.s2[0], forced[-1])
    assert len(np.unique(forced[1:])) == 2 * n_pop


def test_the_population_runs_move(rpl4):
    L, at = rpl4
    runs = [pop_run(L, at, n_pop)[1] for n_pop in POPS] + [pop_run(L, at, 4096, updatesigma=True)[1]]
    moves("populations", runs, nulls=True)      # m0 = 3 < n_pop


# ---------------------------------------------------------------------------------------------------------------------
# archive indices at or above 2^16


def archive_plan(L, c):
    """Four chains on the cell c with ARCHIVE_M0 archive rows: row r is chain r % 4's start plus a uniform draw within
    ARCHIVE_FRACTION of [lower, upper] on either side, clipped into the box."""
    pl = plan(L, (c,), 4, 4)
    P = 7 + int(L.cells.lengths[c])
    assert pl.pop0.shape[2] == P and np.all(np.isfinite(pl.lower[0])) and np.all(np.isfinite(pl.upper[0]))
    rs = np.random.default_rng(SEED)
    width = ARCHIVE_FRACTION * (pl.upper[0] - pl.lower[0])
    z0 = pl.pop0[0][np.arange(ARCHIVE_M0) % 4] + width * rs.uniform(-1.0, 1.0, (ARCHIVE_M0, P))
    z0 = np.clip(z0, pl.lower[0], pl.upper[0])
    return dataclasses.replace(pl, z0=z0[None])


def archive_reach(key, P=9):
    """(the largest row index a chain used, the largest one used in generations 3 and 4) under the stream key, from the
    restatement's index draws: a and c always, e in a snooker move."""
    top = []
    for g in range(1, 5):
        M = O.archive_rows(g, ARCHIVE_M0, 4, ARCHIVE_KW["append_every"])
        a, c, e, _, snk, _ = O.index_draws(SEED, key, g, 4, M, P, ARCHIVE_KW["p_snooker"])
        assert max(a.max(), c.max(), e.max()) < M
        top.append(int(max(a.max(), c.max(), e[snk].max(initial=-1))))
    return max(top), max(top[2:])


def test_archive_rows_at_and_above_2_16(rpl4):
    L, at = rpl4
    pl = archive_plan(L, at[2])
    assert len(np.unique(pl.z0[0], axis=0)) == ARCHIVE_M0            # all rows distinct
    assert np.all(pl.z0[0] >= pl.lower[0]) and np.all(pl.z0[0] <= pl.upper[0])
    got = device(L, pl, keys=[ARCHIVE_KEY], **ARCHIVE_KW)
    assert got.n_archive == ARCHIVE_M0 + 8 == got.archive.shape[1]
    replayed(L, pl, got, 0, 4, key=ARCHIVE_KEY, **ARCHIVE_KW)
    np.testing.assert_array_equal(got.archive[0, :ARCHIVE_M0], pl.z0[0])
    np.testing.assert_array_equal(got.archive[0, ARCHIVE_M0:].reshape(2, 4, 9), got.chain[[2, 4]])
    assert O.archive_rows(3, ARCHIVE_M0, 4, 2) == ARCHIVE_M0 + 4 == O.archive_rows(4, ARCHIVE_M0, 4, 2)
    top, late = archive_reach(ARCHIVE_KEY)
    assert top >= 2 ** 16 and late >= ARCHIVE_M0         # a row appended after generation 2 is read, past 2^16
    assert all(archive_reach(k)[1] < ARCHIVE_M0 for k in range(ARCHIVE_KEY))   # the first such key
    moves("archive", [got], nulls=False)


# ---------------------------------------------------------------------------------------------------------------------
# logs and kept rows


def log_plan(L, at):
    return plan(L, (at[129], at[2]), *LOG_SHAPE)


LOG_KW = dict(n_gen=5, jump_every=3, thin=1, append_every=2, CR=0.3, p_snooker=0.5, archive=True)
_log_runs = {}


def log_run(L, at, **kw):
    key = tuple(sorted(kw.items()))
    if key not in _log_runs:
        _log_runs[key] = device(L, log_plan(L, at), **{**LOG_KW, **kw})
    return _log_runs[key]


@pytest.mark.parametrize("log_rows", [0, 2, 5, 8])
def test_logs_hold_the_leading_generations(rpl4, log_rows):
    L, at = rpl4
    B = 2 * LOG_SHAPE[0]
    full, got = log_run(L, at, log_rows=5), log_run(L, at, log_rows=log_rows)
    G = min(log_rows, 5)
    for f in LOGS:
        assert getattr(got, f).shape == (G, B) and getattr(got, f).dtype == getattr(full, f).dtype
        np.testing.assert_array_equal(getattr(got, f), getattr(full, f)[:G], err_msg=f)
    assert np.any(full.logr[-1] != full.logr[0]) and np.any(full.snooker[-1] != full.snooker[0])
    for f in KEPT + MEMBER + ("archive", "n_archive"):
        np.testing.assert_array_equal(getattr(got, f), getattr(full, f), err_msg=f)


def test_no_kept_rows_and_the_starting_row_alone(rpl4):
    """thin = 0: the device holds no chain and generation 0 keeps nothing; thin = 9 > n_gen: row 0 alone. The sampler's
    path does not depend on what is kept."""
    L, at = rpl4
    n_pop = LOG_SHAPE[0]
    pl = log_plan(L, at)
    kw = dict(updatesigma=True, log_rows=5)
    ref, none, first = log_run(L, at, **kw), log_run(L, at, thin=0, **kw), log_run(L, at, thin=9, **kw)
    assert ref.chain.shape == (6, 2 * n_pop, 136)
    for f in KEPT:
        assert getattr(none, f).shape == (0,) + getattr(ref, f).shape[1:]
        np.testing.assert_array_equal(getattr(first, f), getattr(ref, f)[:1], err_msg=f)
    np.testing.assert_array_equal(first.chain[0], pl.pop0.reshape(2 * n_pop, 136))
    assert np.all(first.s2chain == 1.0) and np.all(ref.s2chain[1:] != 1.0)
    for got in (none, first):
        for f in MEMBER + LOGS + ("archive", "n_archive"):
            np.testing.assert_array_equal(getattr(got, f), getattr(ref, f), err_msg=f)


KEEP_KW = dict(n_gen=7, jump_every=3, thin=3, append_every=2, CR=0.3, p_snooker=0.5, log_rows=7, archive=True)


def test_generations_that_keep_append_do_both_and_do_neither(rpl4):
    """n_gen = 7, thin = 3, append_every = 2: generation 3 keeps only, 2 and 4 append only, 6 does both and 1, 5 and 7
    do neither (k_zs_decide's early return)."""
    L, at = rpl4
    n_pop, m0 = LOG_SHAPE
    pl = log_plan(L, at)
    got = log_run(L, at, **KEEP_KW)
    assert got.chain.shape == (3, 2 * n_pop, 136) and got.n_archive == m0 + 3 * n_pop == got.archive.shape[1]
    for k in range(2):
        want = replayed(L, pl, got, k, n_pop, **KEEP_KW)
        assert want["chain"].shape[0] == 3
    np.testing.assert_array_equal(got.archive[:, m0 + 2 * n_pop:].reshape(2 * n_pop, 136), got.chain[2])   # generation 6


def test_the_log_and_kept_row_runs_move(rpl4):
    L, at = rpl4
    moves("logs and kept rows", [log_run(L, at, log_rows=5), log_run(L, at, updatesigma=True, log_rows=5),
                                 log_run(L, at, **KEEP_KW)], nulls=False)     # m0 = 90 >= n_pop
