"""Input builders for the ragged-context tests (tests/test_ragged_contexts_gpu.py) and the oracle
cross-check that pins their reference (tests/test_oracle_golden.py). Host only: numpy, the package's
data helpers, the construct tables and tests/variant_rows.py; no GPU and no oracle call.

A context picks one likelihood kernel for all its cells from its longest cell (pick_rpl, tci_api.cpp),
so every shorter cell of the table runs on that kernel's padded records: whole lanes hold no real
step, the tail point pt[RPL] does not exist, and the prologue's speculative dR loads read whatever
lies past the row's 7 + N entries. The contexts below hold one cell per length, from 2 points up to
the class's last length, with the lengths on each side of every lane-group, class and tile edge in
between (CONTEXTS). For the lengths in TWIN_LENGTHS a twin cell on t = 0.25 * arange(N) follows, on
which variant_rows.integer_counter_rows applies.

Rows of one cell (row_families), each built for that cell alone and packed to the context's
ld = 7 + N_max:

  random         four draw_x0 rows, the first with v in U(0.05, 0.5) (long windows);
  edge           variant_rows.edge_rows(t);
  on a cut       up to six rows of variant_rows.threshold_rows(cs, [t]) (a position P_m exactly on a
  near a cut     decision threshold) and up to six of its near-integer-quotient rows. They need a step
                 m with 1 <= m < N - 1, so a 2-point cell has none (asserted, not skipped);
  integer counter  variant_rows.integer_counter_rows(N), on the twin cells (which take the random and
                 edge rows beside them, and leave the threshold and non-finite rows to their primary cell:
                 the cap below);
  non-finite scalar / non-finite dR / dR past the last step
                 the non-finite set of tests/test_lk_valu_gpu.py's case(): each of the seven scalars, the
                 first and the last step's dR (index N - 2), and the last rate, which no step reads.

Only "non-finite scalar" and "non-finite dR" give NaN; every other row is a number.
tile_max's 2,048-point cell keeps the random and edge rows only (the oracle's time).
At most MAX_ROWS_PER_CELL rows per cell and MAX_ROWS_PER_CASE per (context, construct).
"""
import dataclasses

import numpy as np

import variant_rows as VR

# context -> (cell lengths, the rows-per-lane class pick_rpl must choose; 0: the long-cell tile kernel).
#   tile:     S = N - 1 on, one before and one after a 64-row tile edge (63 | 64 | 65, 127 | 128 | 129,
#             512 | 513) and a ragged last tile (599);
#   tile_max: the dynamic LDS sized for 2,048 points while a 2-point cell runs in it.
CONTEXTS = {
    "rpl2": ((2, 3, 64, 65, 66, 129), 2),
    "rpl4": ((2, 3, 65, 66, 129, 130, 257), 4),
    "rpl8": ((2, 3, 65, 129, 130, 257, 258, 513), 8),
    "tile": ((2, 3, 63, 64, 65, 66, 128, 129, 130, 513, 514, 600), 0),
    "tile_max": ((2, 65, 2048), 0),
}
TWIN_LENGTHS = (3, 65, 66, 130)
# two_segment and seg4 take the KParams-first prologue (tci_cohort_kernel_k)
CONSTRUCTS_OF = {
    "rpl2": ("builtin",),
    "rpl4": ("builtin", "two_segment", "seg4"),
    "rpl8": ("builtin", "two_segment", "seg4"),
    "tile": ("builtin", "two_segment", "seg4"),
    "tile_max": ("builtin",),
}
CASES = [(ctx, cname) for ctx in CONTEXTS for cname in CONSTRUCTS_OF[ctx]]
LONG_CELL = 2048                   # random and edge rows only
MAX_ROWS_PER_CELL = 60
MAX_ROWS_PER_CASE = 700
MAX_CUT_ROWS = 6                   # per cell, of each threshold family
NAN_FAMILIES = ("non-finite scalar", "non-finite dR")
GARBAGE = (np.nan, np.inf, -1e300)  # what padding_garbage writes, in rotation


def context_cells(ctx):
    """The cell list of a context, [(t, ms2, pp7), ...] in the order of CONTEXTS[ctx] with every twin
    right after its primary cell, and per cell whether it is a twin. Times from synthetic_times, data
    normal with 37 % NaN (variant_rows.synthetic_cell_list); the cells do not depend on the construct."""
    lengths, _ = CONTEXTS[ctx]
    rng = np.random.default_rng(9000 + sum(lengths))
    cl, twin = [], []
    for n in lengths:
        cl += VR.synthetic_cell_list(rng, n, n_cells=1)
        twin.append(False)
        if n in TWIN_LENGTHS:
            y1, y2 = rng.normal(3, 2, n), rng.normal(6, 3, n)
            y1[rng.random(n) < 0.37] = np.nan
            y2[rng.random(n) < 0.37] = np.nan
            cl.append((0.25 * np.arange(n), y1, y2))
            twin.append(True)
    return cl, np.array(twin)


def primary_cells(ctx):
    """point count -> cell index of the context's primary (non-twin) cells, in context_cells' order."""
    lengths, _ = CONTEXTS[ctx]
    out, c = {}, 0
    for n in lengths:
        out[n] = c
        c += 2 if n in TWIN_LENGTHS else 1
    return out


def nonfinite_rows(n):
    """[(row, family)]: tests/test_lk_valu_gpu.py's non-finite set for a cell of n points."""
    base = np.concatenate([[2.0, 1.5, 0.5, 2.0, 1.0, 0.7, 9.0], np.zeros(n)])
    out = []
    for k, val in ((0, np.inf), (1, np.nan), (2, -np.inf), (3, np.nan), (4, np.inf), (5, np.nan), (6, np.inf)):
        r = base.copy()
        r[k] = val
        out.append((r, "non-finite scalar"))
    for j in sorted({0, n - 2}):  # the first and the last step's dR (one entry for a 2-point cell)
        for val in (np.inf, np.nan):
            r = base.copy()
            r[7 + j] = val
            out.append((r, "non-finite dR"))
    for val in (np.inf, np.nan):  # past the last step: no step reads it
        r = base.copy()
        r[7 + n - 1] = val
        out.append((r, "dR past the last step"))
    return out


def _spread(items, count):
    """At most count of items, evenly spaced (first and last kept)."""
    if len(items) <= count:
        return list(items)
    return [items[i] for i in np.unique(np.linspace(0, len(items) - 1, count).round().astype(int))]


def row_families(rng, cs, t, twin):
    """[(row, family)] of one cell with times t."""
    from transcriptioncycleinference_amd.data import draw_x0

    n = len(t)
    out = []
    for k in range(4):
        r = draw_x0(rng, n)
        if k == 0:
            r[0] = rng.uniform(0.05, 0.5)  # slow elongation: long windows
        out.append((r, "random"))
    out += [(r, "edge") for r in VR.edge_rows(t)]
    if n == LONG_CELL:
        return out
    if twin:
        return out + [(r, "integer counter") for r in VR.integer_counter_rows(n)]
    rc, _, _, rd, _ = VR.threshold_rows(cs, [t])
    if n < 3:
        assert not rc and not rd, "a 2-point cell has no step m with 1 <= m < N - 1"
    else:
        assert rc and rd, f"N = {n}: no threshold row inside the v box"
    out += [(r, "on a cut") for r in _spread(rc, MAX_CUT_ROWS)]
    out += [(r, "near a cut") for r in _spread(rd, MAX_CUT_ROWS)]
    return out + nonfinite_rows(n)


@dataclasses.dataclass
class Case:
    ctx: str
    cname: str
    cl: list               # [(t, ms2, pp7)]
    twin: np.ndarray       # per cell
    rpl: int               # the class pick_rpl must choose
    theta: np.ndarray      # [B, ld], zero past a row's 7 + N entries
    cid: np.ndarray        # [B] int32
    what: np.ndarray       # [B] family names
    n: np.ndarray          # [B] points of the row's cell

    @property
    def ld(self):
        return self.theta.shape[1]

    @property
    def finite(self):
        """Rows whose SS is a number (every family but NAN_FAMILIES)."""
        return ~np.isin(self.what, NAN_FAMILIES)


_cases = {}


def case(ctx, cname):
    """The cells and rows of one (context, construct), built once. The arrays are shared: copy before
    changing them."""
    if (ctx, cname) in _cases:
        return _cases[(ctx, cname)]
    cs = VR.matrix_constructs()[cname]
    lengths, rpl = CONTEXTS[ctx]
    cl, twin = context_cells(ctx)
    ld = 7 + max(lengths)
    rng = np.random.default_rng(9100 + sum(lengths) + cs.n_seg)
    rows, cid, what = [], [], []
    for c, (t, _, _) in enumerate(cl):
        fam = row_families(rng, cs, t, bool(twin[c]))
        assert len(fam) <= MAX_ROWS_PER_CELL, (ctx, cname, len(t), len(fam))
        assert all(len(r) == 7 + len(t) for r, _ in fam)
        rows += [r for r, _ in fam]
        what += [w for _, w in fam]
        cid += [c] * len(fam)
    assert len(rows) <= MAX_ROWS_PER_CASE, (ctx, cname, len(rows))
    theta = np.zeros((len(rows), ld))
    for i, r in enumerate(rows):
        theta[i, :len(r)] = r
    cid = np.array(cid, np.int32)
    n = np.array([len(c[0]) for c in cl], np.int64)[cid]
    k = Case(ctx, cname, cl, twin, rpl, theta, cid, np.array(what), n)
    for a in (k.theta, k.cid, k.what, k.n):
        a.setflags(write=False)
    _cases[(ctx, cname)] = k
    return k


def padding_garbage(theta, n):
    """A copy of theta with every entry of row b from index 7 + n[b] - 1 on -- the last rate, which no
    step reads, and the row's padding -- replaced by NaN, +Inf or -1e300 in rotation."""
    out = np.array(theta, np.float64)
    g = np.array(GARBAGE)
    for b in range(len(out)):
        j = np.arange(7 + int(n[b]) - 1, out.shape[1])
        out[b, j] = g[(j + b) % len(g)]
    return out


def shuffle_and_flags(k, seed=5):
    """(order, active): a fixed permutation of the case's rows, so that neighbouring waves hold cells
    of different lengths, and a flag per shuffled row, about 30 % of them 0 (inactive)."""
    rng = np.random.default_rng(seed + len(k.cid))
    order = rng.permutation(len(k.cid))
    active = (rng.random(len(order)) >= 0.3).astype(np.uint8)
    return order, active
