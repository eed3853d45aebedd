"""Every separately compiled likelihood variant against the C oracle on inputs built to need the
fallbacks (needs an MI355X).

tci_cohort_kernel<RPL, NSEG, MODE> (RPL 1/2/4/8, NSEG 1..4, SS / forward-interp / forward-raw) and
tci_tile_kernel<NSEG, MODE> (514-2,048 points, its own restatement of the algorithm) are a matrix of
kernels; tci_diag.h has no counter for the path a wave took, so a proof that wrongly fails to fall
back shows only in the results of rows that need the fallback. tests/variant_rows.py builds those
rows (random, edge, threshold, near-integer quotient, cut boundary; integer loading counters) for any
(N, construct); this module runs them on every (rows-per-lane class, construct) pair and at the tile
kernel's carry edges (S = N - 1 a multiple of 64 and one past it: N = 577, 578, 1025).

Tolerances are those of tests/test_parity_gpu.py: 1e-10 on SS against the oracle, 1e-12 on forward
rows and between the default and the forced-exact paths.
"""
import numpy as np
import pytest

import variant_rows as VR
from conftest import pack

pytestmark = pytest.mark.gpu

REL = 1e-10


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

# N -> the rows-per-lane class pick_rpl must choose (0: the long-cell tile kernel)
RPL_OF_N = {33: 1, 65: 1, 100: 2, 129: 2, 130: 4, 257: 4, 258: 8, 513: 8, 514: 0, 577: 0, 578: 0, 1025: 0}
CONSTRUCTS = ("builtin", "two_segment", "seg3", "seg4")


@pytest.fixture(scope="module")
def constructs():
    return VR.matrix_constructs()


def run_case(n, cs, c_oracle, seed):
    """Three synthetic cells of n points, the five row families on one Likelihood context, against the
    C oracle: SS on the default path, SS on the forced-exact paths, default against forced, and both
    forward grids for the first 6 rows and every eighth row after them. (The interp-grid forward row
    78 of the N = 1025 two-segment case, v = 0.0555, is the one that was 1.92e-12 off while the tile
    kernel's forward rows still took the O(1) row sums: DESIGN.md §5.)"""
    from transcriptioncycleinference_amd import Likelihood, from_lists

    cl, rows, cid, fam, lanes = VR.case_rows(n, cs, seed)
    assert len(rows) < 150
    # the v filter must not hide a variant: enough threshold rows, and every threshold lane hit
    assert (fam == "c").sum() >= 8 and (fam == "d").sum() >= 8, (fam == "c").sum()
    assert set(lanes) == set(range(1 + 4 * cs.n_seg)), sorted(set(lanes))
    cells = from_lists(cl)
    ocs = VR.oracle_construct(cs)
    theta = pack(rows)
    fw = np.concatenate([np.arange(6), np.arange(6, len(rows), 8)])
    with Likelihood(cells, cs, device=0) as L:
        assert L.info["rows_per_lane"] == RPL_OF_N[n]
        ss = L.ss_batch(theta, cid)
        L.set_force_exact(scan=True, positions=True)
        try:
            ss_exact = L.ss_batch(theta, cid)
        finally:
            L.set_force_exact()
        fr = L.forward(theta[fw], cid[fw], grid="raw")
        fi = L.forward(theta[fw], cid[fw], grid="interp")
    want, st = c_oracle.ss_batch(cells.offsets, cells.t, cells.ms2, cells.pp7, ocs, theta, cid)
    assert np.all(st == 0), st[st != 0][:5]
    for f in "abcde":
        k = fam == f
        print(f"N={n} {cs.name} family {f}: {k.sum()} rows, default {rel_err(ss[k], want[k]):.2e}, "
              f"forced exact {rel_err(ss_exact[k], want[k]):.2e}, default vs forced {rel_err(ss[k], ss_exact[k]):.2e}")
    for f in "abcde":
        k = fam == f
        assert rel_err(ss[k], want[k]) <= REL, f"family {f}: default path vs oracle"
        assert rel_err(ss_exact[k], want[k]) <= REL, f"family {f}: forced exact paths vs oracle"
        assert rel_err(ss[k], ss_exact[k]) <= 1e-12, f"family {f}: default vs forced exact"
    worst = 0.0
    for i, b in enumerate(fw):
        t = cells.cell(int(cid[b]))[0]
        for mode, (ms2, pp7) in ((0, fr), (1, fi)):
            m, p = c_oracle.forward(t, ocs, theta[b], mode=mode)
            e = max(rel_err(ms2[i, :n], m), rel_err(pp7[i, :n], p))
            worst = max(worst, e)
            assert e <= 1e-12, f"forward {'raw' if mode == 0 else 'interp'} row {b} (family {fam[b]})"
    print(f"N={n} {cs.name}: {len(fw)} forward rows x 2 grids, max rel err {worst:.2e}")


@pytest.mark.parametrize("cname", CONSTRUCTS)
@pytest.mark.parametrize("n", sorted(RPL_OF_N))
def test_variant_matrix_vs_oracle(n, cname, constructs, c_oracle):
    """tci_cohort_kernel<RPL, NSEG, *> for every RPL and NSEG, two lengths per RPL class (the class's
    first length region and its last length, 64 RPL + 1), and tci_tile_kernel<NSEG, *> at its first
    length and at S = 576, 577 and 1024 (full last tile, one live row in the last tile)."""
    run_case(n, constructs[cname], c_oracle, 1000 + n)


@pytest.mark.parametrize("cname", ["builtin", "two_segment"])
@pytest.mark.parametrize("n", [49, 120, 250, 500, 700])
def test_integer_counters_in_every_variant(n, cname, constructs, c_oracle):
    """dt = 0.25 exactly and R + dR multiples of 4: every loading-counter value is an exact integer, so
    no scan can prove floor() and every wave must take the serial counter (eval_wave's 2^-42 margin, the
    tile kernel's 2^-38 one) -- one cell per RPL class and one on the tile kernel, with rates that change
    inside the cell so the counters cross lane and tile boundaries with different increments. SS and the
    raw-grid forward rows against the oracle."""
    from transcriptioncycleinference_amd import Likelihood, from_lists

    cs = constructs[cname]
    ocs = VR.oracle_construct(cs)
    t = 0.25 * np.arange(n)
    rng = np.random.default_rng(3)
    cells = from_lists([(t, rng.normal(4, 1, n), rng.normal(8, 2, n))])
    rows = VR.integer_counter_rows(n)
    # the non-integer products really are order-sensitive at this length (else the rows prove nothing)
    assert any(VR.order_sensitive_steps(R, n) for R in (0.4, 1.2, 2.8))
    theta = pack(rows)
    cid = np.zeros(len(rows), np.int32)
    with Likelihood(cells, cs, device=0) as L:
        assert L.info["rows_per_lane"] == {49: 1, 120: 2, 250: 4, 500: 8, 700: 0}[n]
        ss = L.ss_batch(theta, cid)
        ms2, pp7 = L.forward(theta, cid, grid="raw")
    want, st = c_oracle.ss_batch(cells.offsets, cells.t, cells.ms2, cells.pp7, ocs, theta, cid)
    assert np.all(st == 0)
    print(f"N={n} {cs.name}: {len(rows)} integer-counter rows, SS max rel err {rel_err(ss, want):.2e}")
    assert rel_err(ss, want) <= REL
    for i in range(len(rows)):
        m, p = c_oracle.forward(t, ocs, theta[i], mode=0)
        assert rel_err(ms2[i, :n], m) <= 1e-12 and rel_err(pp7[i, :n], p) <= 1e-12, f"forward raw row {i}"
