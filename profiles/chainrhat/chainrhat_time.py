"""Time the group reduction (classic and split R-hat, pooled moments) next to what it replaces, and the replicates
themselves next to a one-chain fit.

Two cases, each after a TestData run of 200,000 steps with --replicates chains per cell:
  flagship      299 cells, thin = 100: 2,000 kept rows, the post-burn-in 1,000 of them in the reduction;
  long_columns  a few cells (--long-cells), thin = 1 and stats_from = 10,000: 190,001 rows per column.
For each this measures
  * the kernels alone (HIP events around launch_chainrhat, median and range of the repeats),
  * the device-to-host copy of the same chain rows (torch, pinned host buffer, HIP events),
  * a numpy evaluation of the same statistics on the copied rows (means, variances, the two factors),
  * the run's wall time with the replicates and with one chain per cell (median of three runs each, without the
    copy of the kept rows; with it, as fit() runs, once), and the engine AUTO's rule gives for either (not read from
    the run: the walk engine above two chains per compute unit, tci_api_dram.cpp),
checks the device result against the longdouble restatement of tests/chainrhat_oracle.py within its bound (on
--oracle-groups groups), and writes profiles/chainrhat/chainrhat_time.json.

    python profiles/chainrhat/chainrhat_time.py [--repeats 11] [--steps 200000] [--long-cells 4] [--replicates 4]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import chainrhat_oracle as O  # noqa: E402
from transcriptioncycleinference_amd import Likelihood, testdata  # noqa: E402
from transcriptioncycleinference_amd.mcmc import DramOptions, dram_run, plan_fit, replicate_keys  # noqa: E402


def numpy_rhat(rows, s2, group, M):
    """The statistics the kernels give, the plain numpy way: per chain column mean and var, then the two factors."""
    n = rows.shape[0]
    h = n // 2
    x = np.concatenate([rows, s2[:, :, None]], axis=2)
    out = []
    for seqs, L in (((x,), n), ((x[:h], x[n - h:]), h)):
        mu = np.stack([s.mean(axis=0) for s in seqs], axis=1)          # [chains, seqs, cols]
        var = np.stack([s.var(axis=0, ddof=1) for s in seqs], axis=1)
        K = len(group) // M
        mu = mu.reshape(M, K, -1, mu.shape[-1]).transpose(1, 0, 2, 3).reshape(K, -1, mu.shape[-1])
        var = var.reshape(M, K, -1, var.shape[-1]).transpose(1, 0, 2, 3).reshape(K, -1, var.shape[-1])
        with np.errstate(invalid="ignore", divide="ignore"):
            out.append(np.sqrt((L - 1) / L + mu.var(axis=1, ddof=1) / var.mean(axis=1)))
    return out


def run(lk, cells, ids, o, M, **kw):
    p = plan_fit(cells, ids, 0, replicates=M)
    keys = replicate_keys(ids, M)
    t0 = time.perf_counter()
    res = dram_run(lk, np.tile(np.array(ids, np.int32), M), p.x0, p.lower, p.upper, p.prior_mu, p.prior_sig,
                   p.qcov_diag, 1.0, o, chain_keys=keys, **kw)
    return res, time.perf_counter() - t0


def measure(lk, cells, ids, o, M, repeats, oracle_groups, n_cu):
    K = len(ids)
    group = np.tile(np.arange(K, dtype=np.int32), M)
    run(lk, cells, ids[:2], o, 1, want_chain=False)                      # warm-up: code objects, the engines' graphs
    wall_one = statistics.median(run(lk, cells, ids, o, 1, want_chain=False)[1] for _ in range(3))
    wall_rep = statistics.median(run(lk, cells, ids, o, M, want_chain=False, group=group)[1] for _ in range(3))
    _, wall_one_chain = run(lk, cells, ids, o, 1)
    res, wall_rep_chain = run(lk, cells, ids, o, M, group=group)
    k0 = res.chain.shape[0] - res.rhat.n_rows
    rows, s2 = np.ascontiguousarray(res.chain[k0:]), np.ascontiguousarray(res.s2chain[k0:])
    npar = (7 + cells.lengths[np.tile(ids, M)]).astype(np.int32)
    ms = [res.rhat.kernel_ms]
    for _ in range(max(repeats, 10)):
        cr = lk.chainrhat(rows, s2, npar, group)
        ms.append(cr.kernel_ms)
    assert all(getattr(cr, k).tobytes() == getattr(res.rhat, k).tobytes() for k in O.OUTPUTS)
    dev = torch.from_numpy(rows).cuda()
    host = torch.empty(rows.shape, dtype=torch.float64).pin_memory()
    copy_ms = []
    for _ in range(max(repeats, 10)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        host.copy_(dev, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        copy_ms.append(e0.elapsed_time(e1))
    del dev, host
    t0 = time.perf_counter()
    numpy_rhat(rows, s2, group, M)
    numpy_s = time.perf_counter() - t0
    ng = K if oracle_groups <= 0 else min(oracle_groups, K)
    sel = np.nonzero(group < ng)[0]
    ref = O.table(rows[:, sel], s2[:, sel], npar[sel], group[sel], dtype=O.LD)
    got = {k: v[:ng] for k, v in O.joined(res.rhat).items()}
    try:
        worst, _ = O.check(got, ref, rows.shape[0], "profile")
        checked = "within the bound"
    except AssertionError as e:       # reported, not hidden: the timings below still stand
        worst, checked = {"none": float("nan")}, f"outside the bound: {e}"
    n, nch, ld = rows.shape
    kernel = statistics.median(ms)
    rmax = np.nanmax(np.concatenate([res.rhat.rhat, res.rhat.rhat_split], axis=1), axis=1)
    return {
        "rows": n, "n_chains": nch, "replicates": M, "ld": ld, "chain_bytes": int(rows.nbytes + s2.nbytes),
        "kernel_ms_median": kernel, "kernel_ms_min": min(ms), "kernel_ms_max": max(ms), "repeats": len(ms),
        "d2h_copy_ms_median": statistics.median(copy_ms), "numpy_s": numpy_s,
        "host_route_ms": statistics.median(copy_ms) + 1e3 * numpy_s,
        "kernel_beats_host_route": bool(kernel < statistics.median(copy_ms) + 1e3 * numpy_s),
        "wall_s_one_chain_per_cell": wall_one, "wall_s_replicates": wall_rep, "wall_runs": 3,
        "wall_s_one_chain_per_cell_with_chain_copy": wall_one_chain, "wall_s_replicates_with_chain_copy": wall_rep_chain,
        "auto_engine_by_rule_one_chain_per_cell": "walk" if K > 2 * n_cu else "fused",
        "auto_engine_by_rule_replicates": "walk" if nch > 2 * n_cu else "fused", "compute_units": n_cu,
        "oracle_groups": ng, "oracle_check": checked, "largest_error_over_bound": max(worst.values()),
        "rhat_max_median": float(np.median(rmax)), "rhat_max_largest": float(np.max(rmax)),
        "cells_with_rhat_max_above_1.1": int(np.sum(rmax > 1.1)),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--steps", type=int, default=200000)
    ap.add_argument("--thin", type=int, default=100)
    ap.add_argument("--long-cells", type=int, default=4)
    ap.add_argument("--replicates", type=int, default=4)
    ap.add_argument("--oracle-groups", type=int, default=16)
    a = ap.parse_args()
    cells = testdata()
    n_cu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    out = {}
    with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
        o = DramOptions(n_steps=a.steps, burnintime=a.steps // 2, stats_from=a.steps // 2, thin=a.thin, seed=20201028)
        out["flagship"] = measure(lk, cells, list(range(cells.n_cells)), o, a.replicates, a.repeats, a.oracle_groups, n_cu)
        print(json.dumps(out["flagship"]), flush=True)
        o = DramOptions(n_steps=a.steps, burnintime=a.steps // 20, stats_from=a.steps // 20, thin=1, seed=20201028)
        ids = [int(c) for c in np.linspace(0, cells.n_cells - 1, a.long_cells).round()]
        out["long_columns"] = measure(lk, cells, ids, o, a.replicates, a.repeats, 0, n_cu)
        print(json.dumps(out["long_columns"]), flush=True)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "chainrhat_time.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
