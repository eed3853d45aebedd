"""Short cells in a long cell's context: every likelihood kernel on the whole range of cell lengths it
serves, against the C oracle (needs an MI355X).

A context picks ONE kernel for all its cells from its longest cell (pick_rpl, tci_api.cpp): RPL 1 / 2 /
4 / 8 up to 65 / 129 / 257 / 513 points, tci_tile_kernel past that. Every shorter cell runs on that
kernel's padded records -- whole lanes without a real step, no tail point pt[RPL], dR loads issued before
N is known that read what lies past the row's 7 + N entries -- which the one-length contexts of the other
likelihood tests never do. tests/ragged_cases.py builds five contexts holding cells from 2 points up to
the class's last length (one more with a 2,048-point cell beside a 2-point one) and, per cell, rows that
leave the fast path; tests/test_oracle_golden.py pins the reference on them.

One Likelihood, one oracle call and one default-path evaluation per (context, construct), shared by
the tests and never changed. SS at the project's 1e-10 against the oracle, forward rows at 1e-12; NaN
and Inf must match in kind. A row with a non-finite scalar or step rate is NaN (include/tci.h); the
oracle, which restates MATLAB's nansum, is no reference there.
"""
import numpy as np
import pytest

import ragged_cases as RC
import variant_rows as VR
from test_variant_matrix_gpu import REL, rel_err

pytestmark = pytest.mark.gpu

CASE_IDS = [f"{ctx}-{cname}" for ctx, cname in RC.CASES]


class Ctx:
    def __init__(self, ctx, cname, c_oracle):
        from transcriptioncycleinference_amd import Likelihood, from_lists

        self.k = k = RC.case(ctx, cname)
        self.cs = VR.matrix_constructs()[cname]
        self.ocs = VR.oracle_construct(self.cs)
        self.cells = from_lists(k.cl)
        self.lk = Likelihood(self.cells, self.cs, device=0)
        assert self.lk.info["rows_per_lane"] == k.rpl
        # the reference, once per case and never changed: the oracle's SS; NaN outside the finite box
        want, st = c_oracle.ss_batch(self.cells.offsets, self.cells.t, self.cells.ms2, self.cells.pp7, self.ocs,
                                     k.theta, k.cid)
        assert np.all(st[k.finite] == 0) and np.all(np.isfinite(want[k.finite]))
        self.want = np.where(k.finite, want, np.nan)
        self.want.setflags(write=False)
        # the default paths on the zero-padded rows in the case's own order: what the bit comparisons use
        self.ss = self.lk.ss_batch(k.theta, k.cid)
        self.ss.setflags(write=False)


@pytest.fixture(scope="module")
def ctxs(c_oracle):
    made = {}

    def get(ctx, cname):
        if (ctx, cname) not in made:
            made[(ctx, cname)] = Ctx(ctx, cname, c_oracle)
        return made[(ctx, cname)]

    yield get
    for c in made.values():
        c.lk.close()


def same_bits(a, b):
    """Bitwise equal, any NaN equal to any NaN."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.where(nan, 0.0, a).view(np.int64), np.where(nan, 0.0, b).view(np.int64))


def worst_by_length(label, k, got, want, rows=None):
    """Prints the worst error per cell length, returns the lengths above REL."""
    rows = np.ones(len(k.cid), bool) if rows is None else rows
    bad = []
    for n in sorted(set(k.n.tolist())):
        m = rows & (k.n == n)
        e = rel_err(got[m], want[m])
        print(f"{label} N={n}: {m.sum()} rows, max rel err {e:.2e} ({e / REL:.1e} of REL)")
        if not e <= REL:
            bad.append((n, e))
    return bad


@pytest.mark.parametrize("ctx,cname", RC.CASES, ids=CASE_IDS)
def test_ss_parity_shuffled_with_inactive_rows(ctxs, ctx, cname):
    """Every row of the case in one batch, shuffled so that neighbouring waves (and the four waves of an
    RPL >= 4 block) hold cells of different lengths, about 30 % of the rows flagged inactive: +Inf for
    those, the oracle's SS for the others, NaN outside the finite parameter box -- and, bit for bit, what
    the unshuffled, unflagged batch gave."""
    c = ctxs(ctx, cname)
    k = c.k
    order, active = RC.shuffle_and_flags(k)
    assert 0.2 < 1.0 - active.mean() < 0.4
    assert len(set(k.n[order][:16].tolist())) >= 3   # the first waves already hold different lengths
    got = np.empty(len(order))
    got[order] = c.lk.ss_batch(k.theta[order], k.cid[order], active)
    act = np.empty(len(order), bool)
    act[order] = active != 0
    want = np.where(act, c.want, np.inf)
    bad = worst_by_length(f"{ctx} {cname} SS", k, got, want)
    bad0 = worst_by_length(f"{ctx} {cname} SS (unshuffled, all active)", k, c.ss, c.want)
    assert np.all(np.isposinf(got[~act]))
    assert np.all(np.isnan(got[act & ~k.finite])) and np.all(np.isnan(c.ss[~k.finite]))
    assert np.all(np.isfinite(got[act & k.finite])) and np.all(np.isfinite(c.ss[k.finite]))
    assert not bad and not bad0, (bad, bad0)
    for w in dict.fromkeys(k.what):
        assert rel_err(got[k.what == w], want[k.what == w]) <= REL, w
    assert same_bits(got[act], c.ss[act])


def _forward_rows(k):
    """Two rows of every cell -- the slow random row and the second random row, on a twin cell the first
    integer-counter row -- ordered so that the shortest and the longest cell's rows are neighbours."""
    by_len = sorted(range(len(k.cl)), key=lambda c: len(k.cl[c][0]))
    zig = []
    while by_len:
        zig.append(by_len.pop(0))
        if by_len:
            zig.append(by_len.pop())
    rows = []
    for c in zig:
        mine = np.flatnonzero(k.cid == c)
        second = mine[k.what[mine] == "integer counter"][:1] if k.twin[c] else mine[1:2]
        assert k.what[mine[0]] == "random" and len(second) == 1
        rows += [mine[0], int(second[0])]
    return np.array(rows)


@pytest.mark.parametrize("ctx,cname", RC.CASES, ids=CASE_IDS)
def test_forward_rows_of_short_and_long_cells_side_by_side(ctxs, c_oracle, ctx, cname):
    """forward(grid="raw") and grid="interp" for two rows of every cell in one call each, a 2-point
    cell's rows next to the longest cell's: each row's first N entries against the oracle's forward model
    at 1e-12, and NaN from N on -- no row wrote past its own N values, into its padding or its neighbour."""
    c = ctxs(ctx, cname)
    k = c.k
    rows = _forward_rows(k)
    assert abs(int(k.n[rows[1]]) - int(k.n[rows[2]])) == max(k.n) - min(k.n)
    for mode, grid in ((0, "raw"), (1, "interp")):
        ms2, pp7 = c.lk.forward(k.theta[rows], k.cid[rows], grid=grid)
        assert ms2.shape == pp7.shape == (len(rows), int(max(k.n)))
        worst = {}
        for i, b in enumerate(rows):
            n = int(k.n[b])
            m, p = c_oracle.forward(k.cl[int(k.cid[b])][0], c.ocs, k.theta[b, :7 + n], mode=mode)
            worst[n] = max(worst.get(n, 0.0), rel_err(ms2[i, :n], m), rel_err(pp7[i, :n], p))
            assert np.all(np.isnan(ms2[i, n:])) and np.all(np.isnan(pp7[i, n:])), f"{grid} row {b}: written past N={n}"
        print(f"{ctx} {cname} forward {grid}: " + ", ".join(f"N={n} {e:.1e}" for n, e in sorted(worst.items())))
        assert max(worst.values()) <= 1e-12, (grid, worst)


@pytest.mark.parametrize("ctx,cname", RC.CASES, ids=CASE_IDS)
def test_forced_exact_paths(ctxs, ctx, cname):
    """set_force_exact(scan=True), (positions=True) and both: each within REL of the oracle; the serial
    counter alone gives the default path's bits (test_exact_scan_path_is_bitwise_identical), so it changes
    none beside the exact sweep either, and the exact sweep stays within REL of the default path
    (test_forced_exact_paths_agree)."""
    c = ctxs(ctx, cname)
    k = c.k
    got = {}
    try:
        for name, kw in (("scan", dict(scan=True)), ("positions", dict(positions=True)),
                         ("both", dict(scan=True, positions=True))):
            c.lk.set_force_exact(**kw)
            got[name] = c.lk.ss_batch(k.theta, k.cid)
    finally:
        c.lk.set_force_exact()
    for name, ss in got.items():
        print(f"{ctx} {cname} forced {name}: vs oracle {rel_err(ss, c.want):.2e}, vs default {rel_err(c.ss, ss):.2e}")
    for name, ss in got.items():
        assert not worst_by_length(f"{ctx} {cname} forced {name}", k, ss, c.want), name
        assert rel_err(c.ss, ss) <= REL, name
    assert same_bits(got["scan"], c.ss)
    assert same_bits(got["both"], got["positions"])
    assert same_bits(c.lk.ss_batch(k.theta, k.cid), c.ss)   # the hook is off again


@pytest.mark.parametrize("ctx,cname", RC.CASES, ids=CASE_IDS)
def test_padding_does_not_matter(ctxs, ctx, cname):
    """The same rows with every entry from the unused last rate (index 7 + N - 1) to the end of the row
    replaced by NaN, +Inf or -1e300 in rotation -- all but the first rate of a 2-point cell's row, 512
    entries beside a 513-point cell, what the prologue's speculative dR loads read: the SS bits of the zero-padded rows."""
    c = ctxs(ctx, cname)
    k = c.k
    g = RC.padding_garbage(k.theta, k.n)
    short = k.n == min(k.n)
    assert np.all(~np.isfinite(g[short, 8:]) | (g[short, 8:] == -1e300)) and g.shape[1] - 8 == max(k.n) - 1
    got = c.lk.ss_batch(g, k.cid)
    diff = np.flatnonzero(~((got == c.ss) | (np.isnan(got) & np.isnan(c.ss))))
    assert len(diff) == 0, [(int(k.n[b]), k.what[b], got[b], c.ss[b]) for b in diff[:8]]
    assert same_bits(got, c.ss)


@pytest.mark.parametrize("ctx,cname", RC.CASES, ids=CASE_IDS)
def test_layout_does_not_matter(ctxs, ctx, cname):
    """The same cells in reverse order in a second context (other cell ids, other record bases): the same
    SS bits row for row. For rpl4 also without its 130-point cell (the class stays 4): the other cells'
    bits stay."""
    from transcriptioncycleinference_amd import Likelihood, from_lists

    c = ctxs(ctx, cname)
    k = c.k
    nc = len(k.cl)
    with Likelihood(from_lists(k.cl[::-1]), c.cs, device=0) as L:
        assert L.info["rows_per_lane"] == k.rpl
        got = L.ss_batch(k.theta, (nc - 1 - k.cid).astype(np.int32))
    assert same_bits(got, c.ss)
    if ctx == "rpl4":
        drop = next(i for i in range(nc) if len(k.cl[i][0]) == 130 and not k.twin[i])
        keep = [i for i in range(nc) if i != drop]
        new_id = np.full(nc, -1, np.int32)
        new_id[keep] = np.arange(len(keep), dtype=np.int32)
        rows = k.cid != drop
        with Likelihood(from_lists([k.cl[i] for i in keep]), c.cs, device=0) as L:
            assert L.info["rows_per_lane"] == 4
            got = L.ss_batch(k.theta[rows], new_id[k.cid[rows]])
        assert same_bits(got, c.ss[rows])


@pytest.mark.parametrize("ctx,cname", [p for p in RC.CASES if p[0] in ("rpl4", "tile")],
                         ids=[i for i, p in zip(CASE_IDS, RC.CASES) if p[0] in ("rpl4", "tile")])
def test_short_rows_on_the_device_api(ctxs, ctx, cname):
    """ss_batch_device with ld = 7 + 130, every row of the case shuffled into one batch: rows of cells
    of up to 130 points give the host API's bits for the same rows, rows of longer cells NaN
    (tci_ss_batch_async, include/tci.h). The host API refuses the batch with TCI_ERANGE."""
    import torch

    from transcriptioncycleinference_amd import _lib

    c = ctxs(ctx, cname)
    k = c.k
    ld = 7 + 130
    order, _ = RC.shuffle_and_flags(k)
    theta = np.ascontiguousarray(k.theta[order, :ld])
    cid, n = k.cid[order], k.n[order]
    fits = n <= 130
    assert fits.any() and (~fits).any()
    assert not np.any(k.theta[order][fits][:, ld:])   # the rows that fit lose nothing but zero padding
    dev = torch.device("cuda", 0)
    out = torch.full((len(order),), -123.0, dtype=torch.float64, device=dev)
    c.lk.ss_batch_device(torch.from_numpy(theta).to(dev), torch.from_numpy(cid).to(dev), out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(np.isnan(got[~fits])), got[~fits][:8]
    assert same_bits(got[fits], c.ss[order][fits])
    assert rel_err(got[fits], c.want[order][fits]) <= REL
    with pytest.raises(_lib.TciError) as e:
        c.lk.ss_batch(theta, cid)
    assert e.value.code == _lib.TCI_ERANGE
    assert same_bits(c.lk.ss_batch(k.theta, k.cid), c.ss)   # the context still works after the refusal
