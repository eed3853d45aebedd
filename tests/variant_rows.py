"""Input builders shared by the likelihood variant-matrix tests (tests/test_variant_matrix_gpu.py)
and the oracle cross-check that pins their reference (tests/test_oracle_golden.py). Host only: numpy,
the package's data helpers and the construct tables; no GPU and no oracle call.

Row families of one (N, construct) case -- theta rows built to make the fast path's proofs DECLINE,
so a variant whose proof wrongly succeeds returns a wrong number instead of a lucky right one:

  a  random:     16 draw_x0 rows, every fourth with v in U(0.05, 0.5) (long windows);
  b  edge:       v = 0 / tiny / max, tau and ton extremes, A = 0, basal floors above everything,
                 R = 0, every rate clamped to 0, every rate at its maximum;
  c  threshold:  v that puts a representative position P_m = m*(v*d) exactly on a decision threshold
                 (tci_eval.h distance_cut): every segment's MS2 / PP7 loop start and end, v = x/(m*d),
                 and the gene end L = L0 + tau*v, v = L0/(m*d - tau); m in {1, 3, 10, 25, N - 2};
  d  near:       family c's v times (1 +- 3e-8): x/(v*d) within the reciprocal's error of an integer,
                 where the estimate of the cut is off by one and must be flagged, not trusted;
  e  boundary:   v so small that every cut exceeds every row index (all table reads hit the zero pad),
                 so small that only the lowest threshold is crossed, and so large that nL = 0.

Threshold order (lane j of distance_cuts): 0 -> L, 1 + 4k .. 4 + 4k -> MS2 start, MS2 end, PP7 start,
PP7 end of segment k.
"""
import numpy as np

M_STEPS = (1, 3, 10, 25)          # plus N - 2, per case
NEAR = 3e-8                        # family d's relative offset (v_rcp_f64's error reaches 4.6e-8)
MAX_THRESHOLD_ROWS = 56            # family c's cap: every case stays below 150 rows
V_BOX = 20.0                       # family c / d rows with v outside (0, 20) are dropped


def matrix_constructs():
    """name -> the package's Construct: the built-in one, the 2-segment 3x-length construct and the
    3- and 4-segment constructs of test_multi_segment_constructs_vs_oracle."""
    from transcriptioncycleinference_amd.construct import Construct, builtin_construct, long_two_loop_construct

    out = {"builtin": builtin_construct("P2P-MS2v5-LacZ-PP7v4"), "two_segment": long_two_loop_construct()}
    for nseg in (3, 4):
        a = np.linspace(0.05, 9.0, nseg)
        out[f"seg{nseg}"] = Construct(11.0, list(a), list(a + 0.8), [24.0, 12.0, 6.0, 24.0][:nseg],
                                      list(a + 0.3), list(a + 1.9), [24.0] * nseg, f"seg{nseg}")
    return out


def oracle_construct(cs):
    from oracle import oracle as O

    return O.Construct(cs.L0, cs.ms2_start, cs.ms2_end, cs.ms2_loopn, cs.pp7_start, cs.pp7_end, cs.pp7_loopn)


def thresholds(cs):
    """(lane, value) of every construct threshold, lanes 1 .. 4 * n_seg (lane 0, L, depends on theta)."""
    out = []
    for k in range(cs.n_seg):
        for j, x in enumerate((cs.ms2_start[k], cs.ms2_end[k], cs.pp7_start[k], cs.pp7_end[k])):
            out.append((1 + 4 * k + j, float(x)))
    return out


def synthetic_cell_list(rng, n, n_cells=3, nan_fraction=0.37):
    """n_cells cells of n points: synthetic_times, normal data, 37 % NaN (as
    test_rows_per_lane_variants_vs_oracle)."""
    from transcriptioncycleinference_amd.data import synthetic_times

    cl = []
    for _ in range(n_cells):
        t = synthetic_times(rng, n)
        y1, y2 = rng.normal(3, 2, n), rng.normal(6, 3, n)
        y1[rng.random(n) < nan_fraction] = np.nan
        y2[rng.random(n) < nan_fraction] = np.nan
        cl.append((t, y1, y2))
    return cl


def grid_step(t):
    """The grid increment d = mean(diff(t)) (SumofSquares...m:29), summed as the existing threshold test does."""
    return float(np.sum(np.diff(t))) / (len(t) - 1)


def random_rows(rng, n, n_cells, count=16):
    from transcriptioncycleinference_amd.data import draw_x0

    rows, cid = [], []
    for k in range(count):
        r = draw_x0(rng, n)
        if k % 4 == 0:
            r[0] = rng.uniform(0.05, 0.5)  # slow elongation: long windows
        rows.append(r)
        cid.append(k % n_cells)
    return rows, cid


def edge_rows(t):
    """The row set of test_edge_cases_vs_oracle for a cell with times t."""
    n = len(t)
    base = np.concatenate([[2.0, 1.0, 1.0, 3.0, 2.0, 0.6, 12.0], np.zeros(n)])
    cases = {
        "v=0": {0: 0.0},
        "v tiny": {0: 1e-6},
        "v max": {0: 10.0},
        "tau=0": {1: 0.0},
        "tau max": {1: 20.0},
        "ton after last point": {2: float(t[-1]) + 1.0},
        "ton=0": {2: 0.0},
        "A=0": {5: 0.0},
        "basal huge": {3: 50.0, 4: 50.0},
        "R=0": {6: 0.0},
    }
    rows = []
    for upd in cases.values():
        r = base.copy()
        for k, val in upd.items():
            r[k] = val
        rows.append(r)
    r = base.copy()
    r[7:] = -30.0  # every rate clamped to 0: nothing loads
    rows.append(r)
    r = base.copy()
    r[7:] = 30.0
    r[6] = 40.0
    rows.append(r)
    return rows


def _threshold_row(t, v, tau):
    return np.concatenate([[v, tau, t[0] + 0.5, 1.0, 2.0, 0.7, 9.0], np.zeros(len(t))])


def threshold_rows(cs, times, tau=2.0):
    """Families c and d. Returns (rows_c, cid_c, lanes_c, rows_d, cid_d): at most MAX_THRESHOLD_ROWS
    rows of c, taken threshold by threshold (the step counts m rotate with the lane, so every m is used
    and every lane keeps its share), and for each one row of d with v * (1 + NEAR) or v * (1 - NEAR)
    (both for a one-segment construct, alternating otherwise)."""
    n = len(times[0])
    ms = [m for m in dict.fromkeys(M_STEPS + (n - 2,)) if 1 <= m < n - 1]
    thr = [(0, None)] + thresholds(cs)
    per_lane = max(1, MAX_THRESHOLD_ROWS // len(thr))
    rows_c, cid_c, lanes_c, rows_d, cid_d = [], [], [], [], []
    for lane, x in thr:
        got = 0
        for i in range(len(ms)):
            m = ms[(i + lane) % len(ms)]
            c = (lane + i) % len(times)
            t = times[c]
            d = grid_step(t)
            v = cs.L0 / (m * d - tau) if x is None else x / (m * d)
            if not (0.0 < v < V_BOX):
                continue
            k = len(rows_c)
            rows_c.append(_threshold_row(t, v, tau))
            cid_c.append(c)
            lanes_c.append(lane)
            signs = (1.0, -1.0) if cs.n_seg == 1 else ((1.0,) if k % 2 == 0 else (-1.0,))
            for s in signs:
                rows_d.append(_threshold_row(t, v * (1.0 + s * NEAR), tau))
                cid_d.append(c)
            got += 1
            if got == per_lane:
                break
    return rows_c, cid_c, lanes_c, rows_d, cid_d


def boundary_rows(rng, cs, times):
    """Family e, on cell 0: with S = N - 1 steps of d, P_S = S*v*d is the farthest position.
    v_all: P_S below the lowest threshold (every cut = S); v_one: only the lowest threshold is crossed,
    by the last step alone; v_far / 4 v_far with tau = 0: P_1 = v*d > L = L0, so nL = 0 and every
    construct cut is 0 (the kernels take any finite v; the sampler's box ends at 10)."""
    from transcriptioncycleinference_amd.data import draw_x0

    t = times[0]
    n = len(t)
    d = grid_step(t)
    lo = min(x for _, x in thresholds(cs))
    rows = []
    for v, tau in ((0.5 * lo / ((n - 1) * d), 1.0), (lo / ((n - 1.5) * d), 1.0), (1.25 * cs.L0 / d, 0.0),
                   (5.0 * cs.L0 / d, 0.0)):
        r = draw_x0(rng, n)
        r[0], r[1], r[2] = v, tau, t[0] + 0.3
        rows.append(r)
    return rows


def case_rows(n, cs, seed):
    """The cells and the theta rows of one (N, construct) case: (cell list, rows, cell ids, family of
    every row as one letter, lanes of family c's rows)."""
    rng = np.random.default_rng(seed)
    cl = synthetic_cell_list(rng, n)
    times = [c[0] for c in cl]
    rows, cid = random_rows(rng, n, len(cl))
    fam = ["a"] * len(rows)
    b = edge_rows(times[0])
    rows += b
    cid += [0] * len(b)
    fam += ["b"] * len(b)
    rc, cc, lanes, rd, cd = threshold_rows(cs, times)
    rows += rc + rd
    cid += cc + cd
    fam += ["c"] * len(rc) + ["d"] * len(rd)
    e = boundary_rows(rng, cs, times)
    rows += e
    cid += [0] * len(e)
    fam += ["e"] * len(e)
    return cl, rows, np.array(cid, np.int32), np.array(fam), lanes


def integer_counter_rows(n):
    """Rows of test_integer_counter_forces_exact_fallback (R = 4, dR = 0 on t = 0.25 * arange(n): every
    counter value is an exact integer) plus rows whose R + dR is a multiple of 4 that changes inside the
    cell -- at a third and two thirds of it, around step 64 (a lane-group / tile boundary), and back
    down to 0 -- so the integer counters cross lane and tile boundaries with different increments."""
    rows = []
    for v in (0.5, 1.0, 2.0, 3.0):
        for ton in (0.0, 1.0, 3.3):
            rows.append(np.concatenate([[v, 1.5, ton, 2.0, 1.0, 0.7, 4.0], np.zeros(n)]))
    g = np.arange(n)
    steps = {
        "thirds 4/8/12": 4.0 * (g >= n // 3) + 4.0 * (g >= 2 * n // 3),
        "8 from step 63": 4.0 * (g >= min(63, n // 2)),
        "12 from step 64": 8.0 * (g >= min(64, n // 2 + 1)),
        "16 from step 65, 0 in the last eighth": 12.0 * (g >= min(65, n // 2 + 2)) - 16.0 * (g >= n - n // 8),
        "alternating 4/8": 4.0 * (g % 2),
    }
    for k, dR in enumerate(steps.values()):
        for v, ton in ((1.0, 0.0), (2.5, 1.0 + 0.25 * k)):
            rows.append(np.concatenate([[v, 1.5, ton, 2.0, 1.0, 0.7, 4.0], dR]))
    # Integer-valued products sum exactly in ANY order, so the rows above cannot tell a scan that was
    # wrongly trusted from the serial counter. These can: R * dt = 0.1, 0.3, 0.7 (rounded), whose serial
    # sums land an ulp below or above an integer every few steps (0.1 ten times is 0.9999999999999999)
    # -- floor() then depends on the summation order, and only the reference's serial order is right.
    for R in (0.4, 1.2, 2.8):
        for v, ton in ((1.0, 0.0), (2.0, 1.0)):
            rows.append(np.concatenate([[v, 1.5, ton, 2.0, 1.0, 0.7, R], np.zeros(n)]))
    rows.append(np.concatenate([[1.5, 1.5, 0.5, 2.0, 1.0, 0.7, 0.4], 0.8 * (g >= n // 2) + 1.6 * (g >= 3 * n // 4)]))
    return rows


def order_sensitive_steps(R, n, dt=0.25):
    """Steps at which floor() of the serial counter (ConstantElongationSim.m:60-61) differs from floor()
    of the exactly rounded sum of the same products: where a summation order other than the reference's
    can load a different number of polymerases."""
    import math

    p = R * dt
    counter, out = 0.0, []
    for i in range(1, n):
        counter = counter + p
        if math.floor(counter) != math.floor(math.fsum([p] * i)):
            out.append(i)
    return out
