"""The one-segment RPL <= 2 likelihood kernels after the instruction diet (TCI_LK_VALU, tci_eval.h)
against the C oracle, on the shapes and rows its levers touch (needs an MI355X).

The levers move wave-uniform tests (the finiteness of theta, the prologue's bounds) to the scalar unit,
take the J table entries from the inclusive scan and let the J scan reuse the S scan's zeroed rows. What
they can break shows at the first and last lane, at the tail point, in the second row of a lane, and on
the rows that must leave the fast path -- so: the smallest and largest cell of each rows-per-lane class, and per cell
rows that force the ambiguity path, the exact sweep, v <= 0, the non-finite exits and a ton beyond the
last step. SS at the project's 1e-10 relative bound against the oracle; NaN and Inf must match in kind.

Two cells per context: cell 0 on synthetic_times, cell 1 on t = 0.25 * arange(N), where R * dt can be
made an exact integer. One oracle call per length, shared by the tests.
"""
import numpy as np
import pytest

import variant_rows as VR
from conftest import pack

pytestmark = pytest.mark.gpu

REL = 1e-10
CONSTRUCT = "P2P-MS2v5-LacZ-PP7v4"
RPL_OF_N = {2: 1, 3: 1, 64: 1, 65: 1, 66: 2, 127: 2, 128: 2, 129: 2}


def rel_err(a, b):
    """As tests/test_variant_matrix_gpu.py: max relative error; NaN / Inf must match in kind and sign."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    ok = (np.isnan(a) & np.isnan(b)) | (np.isinf(a) & np.isinf(b) & (np.sign(a) == np.sign(b)))
    with np.errstate(invalid="ignore"):
        d = np.where(ok, 0.0, np.abs(a - b) / np.maximum(np.abs(b), 1e-300))
    d[np.isnan(d)] = np.inf
    return float(np.max(d)) if d.size else 0.0


def case(n):
    """Cells, theta rows, cell ids and a label per row for one length."""
    from transcriptioncycleinference_amd.construct import builtin_construct
    from transcriptioncycleinference_amd.data import draw_x0, synthetic_times

    rng = np.random.default_rng(7000 + n)
    t0, t1 = synthetic_times(rng, n), 0.25 * np.arange(n)
    cl = []
    for t in (t0, t1):
        y1, y2 = rng.normal(3, 2, n), rng.normal(6, 3, n)
        y1[rng.random(n) < 0.3] = np.nan
        y2[rng.random(n) < 0.3] = np.nan
        cl.append((t, y1, y2))
    rows, cid, what = [], [], []

    def add(r, c, w):
        rows.append(np.asarray(r, np.float64))
        cid.append(c)
        what.append(w)

    for k in range(4):
        r = draw_x0(rng, n)
        if k == 0:
            r[0] = rng.uniform(0.05, 0.5)  # slow elongation: long windows
        add(r, k % 2, "random")
    base = np.concatenate([[2.0, 1.5, 0.5, 2.0, 1.0, 0.7, 9.0], np.zeros(n)])
    # R * dt = 1 exactly on cell 1: every counter value is an integer (the ambiguity path); 0.1: serial
    # sums an ulp off an integer every few steps
    for R, v in ((4.0, 1.0), (4.0, 2.5), (0.4, 1.0), (8.0, 0.7)):
        r = base.copy()
        r[0], r[6] = v, R
        add(r, 1, "integer counter")
    r = base.copy()
    r[6] = 4.0
    r[7:] = 4.0 * (np.arange(n) % 2)
    add(r, 1, "integer counter")
    # a position on / within the reciprocal's error of a threshold: the exact sweep
    cs = builtin_construct(CONSTRUCT)
    rc, cc, _, rd, cd = VR.threshold_rows(cs, [t0, t1])
    for r, c in list(zip(rc, cc))[::3][:6]:
        add(r, c, "on a cut")
    for r, c in list(zip(rd, cd))[::5][:6]:
        add(r, c, "near a cut")
    for v in (0.0, -1.0):
        r = base.copy()
        r[0] = v
        add(r, 0, "v <= 0")
    for k, val in ((0, np.inf), (1, np.nan), (2, -np.inf), (3, np.nan), (4, np.inf), (5, np.nan), (6, np.inf)):
        r = base.copy()
        r[k] = val
        add(r, 0, "non-finite scalar")
    for j in sorted({0, n - 2}):  # the first and the last step's dR
        for val in (np.inf, np.nan):
            r = base.copy()
            r[7 + j] = val
            add(r, 0, "non-finite dR")
    for val in (np.inf, np.nan):  # past the last step: no step reads it
        r = base.copy()
        r[7 + n - 1] = val
        add(r, 0, "dR past the last step")
    for c, t in ((0, t0), (1, t1)):
        r = base.copy()
        r[2] = float(t[-1]) + 1.0
        add(r, c, "ton beyond the last step")
    return cl, pack(rows), np.array(cid, np.int32), np.array(what)


class Ctx:
    def __init__(self, n, c_oracle, construct):
        from transcriptioncycleinference_amd import Likelihood, from_lists

        self.n = n
        cl, self.theta, self.cid, self.what = case(n)
        self.cells = from_lists(cl)
        self.lk = Likelihood(self.cells, CONSTRUCT, device=0)
        assert self.lk.info["rows_per_lane"] == RPL_OF_N[n]
        # the reference, once per length and never changed
        self.want, self.st = c_oracle.ss_batch(self.cells.offsets, self.cells.t, self.cells.ms2, self.cells.pp7,
                                               construct, self.theta, self.cid)


@pytest.fixture(scope="module")
def ctxs(c_oracle, construct):
    made = {}

    def get(n):
        if n not in made:
            made[n] = Ctx(n, c_oracle, construct)
        return made[n]

    yield get
    for c in made.values():
        c.lk.close()


@pytest.mark.parametrize("n", sorted(RPL_OF_N))
def test_cell_lengths_and_fallback_rows_vs_oracle(ctxs, n):
    k = ctxs(n)
    ss = k.lk.ss_batch(k.theta, k.cid)
    for w in dict.fromkeys(k.what):
        m = k.what == w
        print(f"N={n} {w}: {m.sum()} rows, max rel err {rel_err(ss[m], k.want[m]):.2e}")
    fin = ~np.isin(k.what, ("non-finite scalar", "non-finite dR"))
    # outside the finite parameter box the kernel reports NaN; everything else is a number
    assert np.all(np.isnan(ss[~fin])), ss[~fin]
    assert np.all(np.isfinite(ss[fin])) and np.all(k.st[fin] == 0)
    for w in dict.fromkeys(k.what[fin]):
        m = k.what == w
        assert rel_err(ss[m], k.want[m]) <= REL, f"N={n} {w}"
    # a dR entry no step reads changes nothing
    m = k.what == "dR past the last step"
    th = k.theta[m].copy()
    th[:, 7 + n - 1] = 0.0
    assert np.array_equal(ss[m], k.lk.ss_batch(th, k.cid[m]))


@pytest.mark.parametrize("n", sorted(RPL_OF_N))
def test_forced_exact_paths_agree(ctxs, n):
    """The serial counter and the exact sweep on every row, against the oracle and the default paths."""
    k = ctxs(n)
    fin = ~np.isin(k.what, ("non-finite scalar", "non-finite dR"))
    ss = k.lk.ss_batch(k.theta[fin], k.cid[fin])
    k.lk.set_force_exact(scan=True, positions=True)
    try:
        exact = k.lk.ss_batch(k.theta[fin], k.cid[fin])
    finally:
        k.lk.set_force_exact()
    print(f"N={n}: forced exact vs oracle {rel_err(exact, k.want[fin]):.2e}, vs default {rel_err(ss, exact):.2e}")
    assert rel_err(exact, k.want[fin]) <= REL
    assert rel_err(ss, exact) <= REL


@pytest.mark.parametrize("n", (65, 129))
def test_mixed_flag_word_and_misaligned_flags(ctxs, n):
    """One word with flags 1,0,1,0, aligned and offset by one byte: rejected rows return +Inf, the others
    the oracle's value."""
    import torch

    k = ctxs(n)
    dev = torch.device("cuda", 0)
    pick = np.flatnonzero(k.what == "random")[:4]
    theta = torch.from_numpy(np.ascontiguousarray(k.theta[pick])).to(dev)
    cid = torch.from_numpy(k.cid[pick]).to(dev)
    flags = np.array([1, 0, 1, 0], np.uint8)
    want = np.where(flags != 0, k.want[pick], np.inf)
    buf = torch.zeros(8, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 4 == 0
    for off in (0, 1):
        buf[off:off + 4] = torch.from_numpy(flags).to(dev)
        out = torch.full((4,), -123.0, dtype=torch.float64, device=dev)
        k.lk.ss_batch_device(theta, cid, out, buf[off:off + 4])
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.all(np.isposinf(got[flags == 0])), got
        assert rel_err(got, want) <= REL, f"N={n} flags at byte offset {off}: {got} vs {want}"


def test_forward_modes(ctxs, construct, c_oracle):
    """forward(grid="interp") and the raw grid at N = 129 (the tail point, both rows of a lane)."""
    k = ctxs(129)
    pick = np.flatnonzero(np.isin(k.what, ("random", "integer counter", "on a cut", "v <= 0")))
    for mode, grid in ((0, "raw"), (1, "interp")):
        ms2, pp7 = k.lk.forward(k.theta[pick], k.cid[pick], grid=grid)
        worst = 0.0
        for i, b in enumerate(pick):
            t = k.cells.cell(int(k.cid[b]))[0]
            m, p = c_oracle.forward(t, construct, k.theta[b], mode=mode)
            worst = max(worst, rel_err(ms2[i, :129], m), rel_err(pp7[i, :129], p))
        print(f"N=129 forward {grid}: {len(pick)} rows, max rel err {worst:.2e}")
        assert worst <= REL


def test_two_segment_construct_at_two_rows_per_lane(c_oracle):
    """The ungated two-segment variant still agrees: one row on a 100-point cell."""
    from transcriptioncycleinference_amd import Likelihood, from_lists, long_two_loop_construct
    from transcriptioncycleinference_amd.data import draw_x0, synthetic_times

    rng = np.random.default_rng(11)
    n = 100
    cells = from_lists([(synthetic_times(rng, n), rng.normal(3, 2, n), rng.normal(6, 3, n))])
    cs = long_two_loop_construct()
    theta = pack([draw_x0(rng, n)])
    cid = np.zeros(1, np.int32)
    with Likelihood(cells, cs, device=0) as L:
        assert L.info["rows_per_lane"] == 2
        ss = L.ss_batch(theta, cid)
    want, st = c_oracle.ss_batch(cells.offsets, cells.t, cells.ms2, cells.pp7, VR.oracle_construct(cs), theta, cid)
    assert np.all(st == 0)
    print(f"two segments, N={n}: rel err {rel_err(ss, want):.2e}")
    assert rel_err(ss, want) <= REL
