"""The mode search's kernels (k_ms_trial / k_ms_select, tci_modesearch.hip) at the shapes tests/test_modesearch_gpu.py
leaves out: populations past one trip of k_ms_select's 1,024-thread member loop and up to the 4,096 its tables hold,
the least-f scan where the winner is a lane's 17th entry, and rows of P = 9 and P = 2055. The method is that module's:
the numpy restatement (tests/modesearch_oracle.py) with Likelihood.ss_batch as its SS function, every output compared
bit for bit. The cells are tests/ragged_cases.py's "rpl4" context (2 to 257 points, rows_per_lane 4) and "tile_max"
(2, 65 and 2,048 points, the tile kernel)."""
import numpy as np
import pytest

import modesearch_oracle as O
import ragged_cases as RC
from test_modesearch_gpu import FIELDS, assert_cell, device, oracle_cell, population

pytestmark = pytest.mark.gpu

PAD = 7.0    # written into pop0's padding: a member's padding is its parent's, never the kernel's


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


def same_cell(a, ka, b, kb, P):
    """Cell ka of run a and cell kb of run b hold the same bits (the rows up to P: the two runs may differ in ld)."""
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        x, y = (x[:, ka], y[:, kb]) if f in ("f_trace", "n_accepted") else (x[ka], y[kb])
        if f in ("pop", "theta_best"):
            x, y = x[..., :P], y[..., :P]
        np.testing.assert_array_equal(x, y, err_msg=f)


@pytest.mark.parametrize("n_pop", [1023, 1024, 1025, 2049, 4096])
def test_large_populations_replay_bit_for_bit(rpl4, n_pop):
    """One, one and a bit, two and a bit and four trips of k_ms_select's member loop; 4,096 fills sh_f and sh_take and
    gives wave 0's scan 64 entries per lane. The 2-point cell (P = 9) and the 65-point cell (P = 72) in one call: two
    workgroups of different P, the short one with ld > P."""
    L, at = rpl4
    sp = population(L.cells, (at[2], at[65]), n_pop)
    assert sp.pop0.shape == (2, n_pop, 72)
    got = device(L, sp, n_gen=2, CR=0.9)
    assert got.n_evals == 2 * n_pop * 3
    for k in range(2):
        want = oracle_cell(L, sp, k, key=k, n_gen=2, CR=0.9)
        assert_cell(got, k, want, 2)
        assert got.best[k] == want["best"] == O.best_index(got.f[k])
        np.testing.assert_array_equal(got.theta_best[k], want["theta_best"])
    print(f"n_pop {n_pop}: accepted {got.n_accepted.tolist()}, best {got.best.tolist()}")
    assert got.n_accepted.sum() > 0
    assert np.all(np.diff(got.f_trace, axis=0) <= 0)


def test_equal_least_members_give_the_least_index(rpl4):
    """2,050 members of the 2-point cell, some of them copies of one row, the best of an ordinary population: the scan
    must return the least index among the equal least f. With the copies at 1029 and 2049 only, the winner is past the
    first trip of the member loop (1029 = 1024 + 5) and the 17th entry of lane 5 (1029 = 5 + 16 * 64)."""
    L, at = rpl4
    n_pop = 2050
    sp = population(L.cells, (at[2],), n_pop)
    plain = device(L, sp, n_gen=0)
    m = int(plain.best[0])
    assert np.sum(plain.f[0] == plain.f[0, m]) == 1     # an ordinary population has one best member
    row, filler = sp.pop0[0, m].copy(), sp.pop0[0, 1 if m == 0 else 0].copy()

    def with_copies(at_rows):
        pop0 = sp.pop0.copy()
        pop0[0, m] = filler
        pop0[0, list(at_rows)] = row
        return type(sp)(**{**sp.__dict__, "pop0": pop0})

    four = with_copies((5, 69, 1029, 2049))
    got = device(L, four, n_gen=0)
    assert got.best[0] == 5
    f4 = got.f[0, [5, 69, 1029, 2049]]
    assert np.all(f4.view(np.int64) == f4.view(np.int64)[0]) and f4[0] == plain.f[0, m]
    assert np.sum(got.f[0] == f4[0]) == 4 and np.all(got.f[0] >= f4[0])
    two = device(L, with_copies((1029, 2049)), n_gen=0)
    assert two.best[0] == 1029 and two.f_trace[0, 0] == f4[0]
    np.testing.assert_array_equal(two.theta_best[0], row)
    moved = device(L, four, n_gen=2)
    want = oracle_cell(L, four, 0, key=0, n_gen=2)
    assert_cell(moved, 0, want, 2)
    assert moved.best[0] == O.best_index(want["f"])


@pytest.mark.parametrize("n_points, n_pop", [(2048, 4), (257, 8)])
def test_long_rows_replay_bit_for_bit(rpl4, tile_max, n_points, n_pop):
    """P = 2055 on the tile kernel (33 trips of the trial kernel's coordinate loop, the crossover counter up to
    i * 2048 + 1027) and P = 264 on an rpl4 context, each cell alone."""
    L, at = tile_max if n_points == 2048 else rpl4
    sp = population(L.cells, (at[n_points],), n_pop)
    assert sp.pop0.shape[2] == 7 + n_points
    got = device(L, sp, n_gen=2)
    assert_cell(got, 0, oracle_cell(L, sp, 0, key=0, n_gen=2), 2)


def test_a_two_point_cell_beside_a_2048_point_cell(tile_max):
    """P = 9 beside P = 2055 in ld = 2055: both replay, the short cell's 2,046 padding columns stay its parents', its
    theta_best is NaN there, and its bits are those of a run of it alone at ld = 9 under the same key."""
    L, at = tile_max
    sp = marked_padding(L, population(L.cells, (at[2048], at[2]), 4))
    assert sp.pop0.shape[2] == 2055 and np.all(sp.pop0[1, :, 9:] == PAD)
    got = device(L, sp, n_gen=2)
    for k in range(2):
        assert_cell(got, k, oracle_cell(L, sp, k, key=k, n_gen=2), 2)
    assert np.all(got.pop[1, :, 9:] == PAD)
    assert np.all(np.isnan(got.theta_best[1, 9:])) and not np.any(np.isnan(got.theta_best[1, :9]))
    alone = device(L, population(L.cells, (at[2],), 4), n_gen=2, keys=[1])
    assert alone.pop.shape[2] == 9
    same_cell(alone, 0, got, 1, 9)
