"""The likelihood kernels' prologue on tiny batches (needs an MI355X).

The prologue of tci_cohort_kernel decides, before any arithmetic, what a row is: past the batch,
bounds-rejected (its flag, read as a 4-byte word or as a byte), a bad cell id, too short for its cell,
or a row to evaluate -- and for the one-segment variants it reads the cell id, the flag word and the
cell table's addresses in one batch of scalar loads, with the row-addressing kernel arguments
delivered in SGPRs. A wrong argument order, a flag word taken from the wrong place or a table address
used before it arrived shows on any row, so the batches here are 1 to 8 rows (every row its own
workgroup for RPL <= 2 and the long-cell kernel, one or two 4-wave workgroups for RPL = 4), one
context per kernel family: three TestData cells (RPL = 2), one synthetic cell each for RPL = 1, RPL = 4
and the long-cell kernel (tci_tile_kernel, N > 513).

Rows go through the device entry point (ss_batch_device), which passes cell ids and the row length to
the kernel unchecked. Expected values: the C oracle (oracle/c_oracle.py) at the tolerance of
tests/test_parity_gpu.py (REL on SS, 1e-12 on forward rows); rejected rows are exactly +Inf, rows with
a bad cell id or shorter than 7 + N are NaN, and no row's neighbour changes.
"""
import numpy as np
import pytest

from conftest import pack

pytestmark = pytest.mark.gpu

REL = 1e-10
CONSTRUCT = "P2P-MS2v5-LacZ-PP7v4"
SENTINEL = -123.0  # what `out` holds before a launch: every row must be written
# kind -> (points of the synthetic cell, the rows-per-lane class the context must pick; 0: tile kernel)
SYNTHETIC = {"rpl1": (40, 1), "rpl4": (200, 4), "tile": (600, 0)}
KINDS = ("rpl1", "rpl2", "rpl4", "tile")
BATCHES = (1, 3, 5, 8)


def rel_err(a, b):
    """As tests/test_parity_gpu.py: max relative error; NaN / Inf must match in kind and sign."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    both_inf = np.isinf(a) & np.isinf(b) & (np.sign(a) == np.sign(b))
    ok = both_nan | both_inf
    with np.errstate(invalid="ignore"):
        d = np.where(ok, 0.0, np.abs(a - b) / np.maximum(np.abs(b), 1e-300))
    d[np.isnan(d)] = np.inf
    return float(np.max(d)) if d.size else 0.0


class Case:
    """One context, 8 rows of it and their oracle SS (computed once, never changed)."""

    def __init__(self, kind, testdata_cells, construct, c_oracle):
        from transcriptioncycleinference_amd import Likelihood, from_lists
        from transcriptioncycleinference_amd.data import draw_x0, synthetic_times

        rng = np.random.default_rng(sum(map(ord, kind)))
        if kind == "rpl2":
            lens = testdata_cells.lengths
            ids = [int(np.argmin(lens)), int(np.argmax(lens)), 0]  # the shortest and the longest cell
            self.cells, rpl = testdata_cells.subset(ids), 2
        else:
            n, rpl = SYNTHETIC[kind]
            y1, y2 = rng.normal(3, 2, n), rng.normal(6, 3, n)
            y1[rng.random(n) < 0.37] = np.nan
            y2[rng.random(n) < 0.37] = np.nan
            self.cells = from_lists([(synthetic_times(rng, n), y1, y2)])
        self.n = [int(x) for x in self.cells.lengths]
        self.cid = (np.arange(8) % self.cells.n_cells).astype(np.int32)
        self.rows = [draw_x0(rng, self.n[c]) for c in self.cid]
        self.theta = pack(self.rows)  # ld = 7 + the longest cell: longer than 7 + N for the shorter ones
        self.construct = construct
        self.c_oracle = c_oracle
        self.want = self.oracle(self.theta, self.cid)
        assert np.all(np.isfinite(self.want))
        self.lk = Likelihood(self.cells, CONSTRUCT, device=0)
        assert self.lk.info["rows_per_lane"] == rpl

    def oracle(self, theta, cid):
        c = self.cells
        ss, st = self.c_oracle.ss_batch(c.offsets, c.t, c.ms2, c.pp7, self.construct, theta, cid)
        assert np.all(st == 0), st[st != 0][:5]
        return ss

    def run(self, theta, cid, active=None):
        import torch

        dev = torch.device("cuda", 0)
        th = torch.from_numpy(np.ascontiguousarray(theta, np.float64)).to(dev)
        ci = torch.from_numpy(np.ascontiguousarray(cid, np.int32)).to(dev)
        ac = None if active is None else torch.from_numpy(np.ascontiguousarray(active, np.uint8)).to(dev)
        out = torch.full((len(cid) + 2,), SENTINEL, dtype=torch.float64, device=dev)
        self.lk.ss_batch_device(th, ci, out[:len(cid)], ac)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.all(got[len(cid):] == SENTINEL), "wrote past the batch"
        return got[:len(cid)]


@pytest.fixture(scope="module")
def cases(cells, construct, c_oracle):
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = Case(kind, cells, construct, c_oracle)
        return made[kind]

    yield get
    for c in made.values():
        c.lk.close()


def check(got, want, what):
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), f"{what}: rejected rows must be exactly +Inf, got {got[inf]}"
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN rows {got} vs {want}"
    e = rel_err(got, want)
    print(f"{what}: max rel err {e:.2e}")
    assert e <= REL, f"{what}: {got} vs {want}"


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("kind", KINDS)
def test_flags_none_all_rejected_and_mixed(cases, kind, B):
    k = cases(kind)
    theta, cid, want = k.theta[:B], k.cid[:B], k.want[:B]
    check(k.run(theta, cid), want, f"{kind} B={B} active=None")
    check(k.run(theta, cid, np.ones(B, np.uint8)), want, f"{kind} B={B} all active")
    check(k.run(theta, cid, np.zeros(B, np.uint8)), np.full(B, np.inf), f"{kind} B={B} all rejected")
    for first in (0, 1):  # rejected rows between live ones, both phases; a non-1 flag byte is active
        act = ((np.arange(B) + first) % 2).astype(np.uint8) * 255
        check(k.run(theta, cid, act), np.where(act != 0, want, np.inf), f"{kind} B={B} mixed from {first}")


@pytest.mark.parametrize("kind", KINDS)
def test_bad_cell_ids_give_nan_beside_valid_rows(cases, kind):
    k = cases(kind)
    for B in (3, 5, 8):
        cid = k.cid[:B].copy()
        bad = [1] if B == 3 else [0, B - 2]
        cid[bad[0]] = -1
        cid[bad[-1]] = k.cells.n_cells if len(bad) > 1 else -1
        want = k.want[:B].copy()
        want[bad] = np.nan
        check(k.run(k.theta[:B], cid), want, f"{kind} B={B} bad ids, active=None")
        act = np.ones(B, np.uint8)
        act[bad[0]] = 0  # a rejected row is +Inf whatever its cell id
        act[B - 1] = 0
        w = want.copy()
        w[act == 0] = np.inf
        check(k.run(k.theta[:B], cid, act), w, f"{kind} B={B} bad ids, flags")
    far = k.cid[:5].copy()
    far[2] = 2**31 - 1
    far[4] = -2**31
    want = k.want[:5].copy()
    want[[2, 4]] = np.nan
    check(k.run(k.theta[:5], far), want, f"{kind} extreme ids")


@pytest.mark.parametrize("kind", KINDS)
def test_row_length_longer_and_shorter_than_the_cell(cases, kind):
    k = cases(kind)
    B = 5
    ld = k.theta.shape[1]
    wide = np.full((B, ld + 5), np.nan)  # the entries past 7 + N are never used
    for b in range(B):
        wide[b, :len(k.rows[b])] = k.rows[b]
    check(k.run(wide, k.cid[:B]), k.want[:B], f"{kind} ld = longest + 5")
    # ld one short of the longest cell: its rows are NaN, shorter cells' rows are evaluated
    short = np.ascontiguousarray(k.theta[:B, :ld - 1])
    want = np.where(np.array([7 + k.n[c] for c in k.cid[:B]]) > ld - 1, np.nan, k.want[:B])
    assert np.isnan(want).any()
    check(k.run(short, k.cid[:B]), want, f"{kind} ld = longest - 1")
    act = np.array([1, 0, 1, 0, 1], np.uint8)
    check(k.run(short, k.cid[:B], act), np.where(act != 0, want, np.inf), f"{kind} ld = longest - 1, flags")


@pytest.mark.parametrize("kind", KINDS)
def test_forward_modes_on_one_row(cases, kind):
    k = cases(kind)
    for b in (0, 1):
        c = int(k.cid[b])
        t = k.cells.cell(c)[0]
        for mode, grid in ((0, "raw"), (1, "interp")):
            ms2, pp7 = k.lk.forward(k.theta[b:b + 1], k.cid[b:b + 1], grid=grid)
            m, p = k.c_oracle.forward(t, k.construct, k.theta[b], mode=mode)
            e = max(rel_err(ms2[0, :len(t)], m), rel_err(pp7[0, :len(t)], p))
            print(f"{kind} row {b} forward {grid}: max rel err {e:.2e}")
            assert e <= 1e-12
