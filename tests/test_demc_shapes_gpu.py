"""The DE-MC kernels (k_demc_propose / k_demc_decide, tci_demc.hip) at the shapes tests/test_demc_gpu.py leaves out:
populations past one trip of k_demc_decide's 1,024-thread loop over the moving members and up to the 2,048 movers its
sh_take holds, odd populations whose half-sweeps move different counts, the Gamma streams at member indices up to 2,049
(i << 16 up to 2^27), and rows of P = 9, 137, 264 and 2055 (1 to 33 bits of the lane's crossing mask). The method is
that module's: the numpy restatement (tests/demc_oracle.py) with Likelihood.ss_batch as its SS function, every output
compared bit for bit, every decision decidable. The cells are tests/ragged_cases.py's "rpl4" context (2 to 257 points,
rows_per_lane 4) and "tile_max" (2, 65 and 2,048 points, the tile kernel)."""
import numpy as np
import pytest

import demc_oracle as O
import ragged_cases as RC
from test_demc_gpu import KEPT, LOGS, MEMBER, S2_RTOL, assert_cell, cell_view, jitter_of, population

pytestmark = pytest.mark.gpu

PAD = 7.0        # written into pop0's padding: a member's padding is its parent's, never the kernel's
# The sampler's seed of every run here. A replay needs every u < exp(logr) decidable (demc_oracle.EXP_MARGIN, 1.8e-15
# relative): the large runs take 2 * n_pop decisions each, 4,098 to 8,192, 24,580 over the four, of which the ones with
# logr < 0 and in bounds draw a uniform; an undecidable one has a chance of about 4e-15 each, so the first seed tried
# serves. Were one to turn up (the tests assert undecided == []), take the next seed.
SEED = 11


def context(name):
    from transcriptioncycleinference_amd import Likelihood, from_lists

    L = Likelihood(from_lists(RC.context_cells(name)[0], name), "P2P-MS2v5-LacZ-PP7v4", device=0)
    assert L.info["rows_per_lane"] == RC.CONTEXTS[name][1]
    at = RC.primary_cells(name)
    assert all(int(L.cells.lengths[c]) == n for n, c in at.items())
    return L, at


@pytest.fixture(scope="module")
def rpl4():
    L, at = context("rpl4")
    with L:
        yield L, at


@pytest.fixture(scope="module")
def tile_max():
    L, at = context("tile_max")
    with L:
        yield L, at


def marked_padding(L, sp):
    """sp with PAD in every member's entries past its cell's P."""
    pop0 = sp.pop0.copy()
    for k, c in enumerate(sp.cells):
        pop0[k, :, 7 + int(L.cells.lengths[c]):] = PAD
    return type(sp)(**{**sp.__dict__, "pop0": pop0})


def device(L, sp, jit, keys=None, **kw):
    kw.setdefault("updatesigma", False)
    return L.demc(sp.pop0, np.array(sp.cells, np.int32), sp.lower, sp.upper, sp.prior_mu, sp.prior_sig, jit, seed=SEED,
                  keys=keys, **kw)


def oracle_cell(L, sp, jit, k, key, **kw):
    c = sp.cells[k]
    P = 7 + int(L.cells.lengths[c])
    return O.run(lambda rows: L.ss_batch(rows, np.full(len(rows), c, np.int32)), sp.pop0[k], P, sp.lower[k], sp.upper[k],
                 sp.prior_mu[k], sp.prior_sig[k], jit[k], key=key, seed=SEED, **kw)


LARGE = (2049, 2050, 4095, 4096)   # movers per half-sweep: 1025 | 1024, 1025 | 1025, 2048 | 2047, 2048 | 2048
LARGE_KW = dict(n_gen=2, thin=1, jump_every=2, CR=0.3)   # the second generation is a jump


@pytest.fixture(scope="module")
def large(rpl4):
    """n_pop -> (device run, restatement) on the 2-point cell (P = 9), jitter at 40 times the default so that trials
    leave the box."""
    L, at = rpl4
    out = {}
    for n_pop in LARGE:
        sp = population(L.cells, (at[2],), n_pop)
        jit = jitter_of(L.cells, sp, 40.0)
        out[n_pop] = device(L, sp, jit, log_rows=2, **LARGE_KW), oracle_cell(L, sp, jit, 0, key=0, **LARGE_KW)
    return out


@pytest.mark.parametrize("n_pop", LARGE)
def test_large_and_odd_populations_replay_bit_for_bit(large, n_pop):
    got, want = large[n_pop]
    assert got.chain.shape == (3, n_pop, 9) and got.logr.shape == (2, n_pop)
    assert want["undecided"] == [], "pick another SEED"
    assert_cell(got, 0, want, n_pop)
    assert np.all(got.n_evals == 1 + 2 - got.n_oob)
    np.testing.assert_array_equal(got.chain[-1], got.pop.reshape(n_pop, 9))


def test_the_large_runs_accept_reject_and_leave_the_box(large):
    acc = rej = oob = 0
    for n_pop, (g, _) in large.items():
        a, o = int(g.accepted.sum()), int(g.trial_oob.sum())
        print(f"n_pop {n_pop}: {a} accepts, {2 * n_pop - a - o} rejects, {o} out of bounds of {2 * n_pop} decisions")
        acc, rej, oob = acc + a, rej + 2 * n_pop - a - o, oob + o
        assert np.all(np.isnan(g.logr) == (g.trial_oob == 1)) and not np.any(g.accepted & g.trial_oob)
    assert acc > 0 and rej > 0 and oob > 0


def test_gamma_streams_of_2050_members(rpl4):
    """updatesigma = 1 with 2,050 members: the restatement's decisions forced on the device's own s2chain, each of its
    s2 draws (Philox and Marsaglia-Tsang restated in Python, stream base i << 16 up to 2^27) held to the device's within
    S2_RTOL, and no two members sharing a stream."""
    L, at = rpl4
    n_pop = 2050
    sp = population(L.cells, (at[2],), n_pop)
    jit = jitter_of(L.cells, sp)
    kw = dict(n_gen=2, jump_every=2, thin=1, CR=0.3, updatesigma=True)
    got = device(L, sp, jit, log_rows=2, **kw)
    forced = cell_view(got, "s2chain", 0, n_pop)
    want = oracle_cell(L, sp, jit, 0, key=0, forced_s2=forced, **kw)
    assert want["undecided"] == [], "pick another SEED"
    np.testing.assert_array_equal(forced[0], np.ones(n_pop))
    np.testing.assert_allclose(forced[1:], want["s2_draw"], rtol=S2_RTOL, atol=0)
    assert_cell(got, 0, want, n_pop, fields=("chain", "sschain", "prichain", "pop", "ss", "accept_rate", "n_oob") + LOGS)
    assert len(np.unique(forced[1:])) == 2 * n_pop


LONG_KW = dict(n_gen=3, thin=1, jump_every=3)


def long_case(L, ids, CR):
    """(plan, jitter, device run) of the cells ids in one call: 5 members, 3 generations, the last one a jump."""
    sp = marked_padding(L, population(L.cells, ids, 5))
    jit = jitter_of(L.cells, sp)
    return sp, jit, device(L, sp, jit, CR=CR, log_rows=3, **LONG_KW)


def replays(L, sp, jit, got, CR):
    for k in range(len(sp.cells)):
        want = oracle_cell(L, sp, jit, k, key=k, CR=CR, **LONG_KW)
        assert want["undecided"] == [], f"cell {k}: pick another SEED"
        assert_cell(got, k, want, 5)
        P = 7 + int(L.cells.lengths[sp.cells[k]])
        rows = cell_view(got, "chain", k, 5)
        if CR == 0.0:   # d' = 1: a member that moved in generation 1 moved in jrand's coordinate alone
            assert np.all(np.sum(rows[1, :, :P] != rows[0, :, :P], axis=1) <= 1)
        print(f"P {P}, CR {CR}: {int(cell_view(got, 'accepted', k, 5).sum())} accepts, "
              f"{int(cell_view(got, 'trial_oob', k, 5).sum())} out of bounds of 15 decisions")


def short_cell_alone(L, sp, jit, got, k, CR):
    """Cell k of the mixed call against a run of it alone at ld = P under the same key; its padding in the mixed call is
    the parents'."""
    c = sp.cells[k]
    P = 7 + int(L.cells.lengths[c])
    one = population(L.cells, (c,), 5)
    assert one.pop0.shape[2] == P < sp.pop0.shape[2]
    alone = device(L, one, jitter_of(L.cells, one), keys=[k], CR=CR, log_rows=3, **LONG_KW)
    for f in KEPT + MEMBER + LOGS:
        a, b = cell_view(alone, f, 0, 5), cell_view(got, f, k, 5)
        if f in ("chain", "pop"):
            b = b[..., :P]
        np.testing.assert_array_equal(a, b, err_msg=f)
    assert np.all(got.pop[k, :, P:] == PAD) and np.all(cell_view(got, "chain", k, 5)[..., P:] == PAD)


@pytest.mark.parametrize("CR", [0.0, 1.0])
def test_2048_point_cell_replays_bit_for_bit(tile_max, CR):
    """P = 2055: 33 bits of the crossing mask in use. CR = 1 sets them all; CR = 0 sets jrand's alone."""
    L, at = tile_max
    sp, jit, got = long_case(L, (at[2048],), CR)
    assert got.chain.shape == (4, 5, 2055)
    replays(L, sp, jit, got, CR)


@pytest.mark.parametrize("CR", [0.0, 1.0])
def test_a_two_point_cell_beside_a_2048_point_cell(tile_max, CR):
    L, at = tile_max
    sp, jit, got = long_case(L, (at[2048], at[2]), CR)
    assert got.chain.shape == (4, 10, 2055)
    replays(L, sp, jit, got, CR)
    short_cell_alone(L, sp, jit, got, 1, CR)


@pytest.mark.parametrize("CR", [0.0, 1.0])
def test_130_and_257_point_cells_on_an_rpl4_context(rpl4, CR):
    L, at = rpl4
    sp, jit, got = long_case(L, (at[130], at[257]), CR)
    assert got.chain.shape == (4, 10, 264)
    replays(L, sp, jit, got, CR)
    short_cell_alone(L, sp, jit, got, 0, CR)
