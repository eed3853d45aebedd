"""Time the log-posterior trace (tci_chainlp) next to what a user does today for the same result, and record what it
says about the replicates of a TestData fit.

Two shapes, each the kept rows of a TestData run of --steps steps (one chain per cell):
  flagship      all 299 cells, thin = 100, the rows past the first half: 1,000 rows per chain;
  long_columns  --long-cells cells, thin = 1, the rows past the first twentieth: 190,001 rows per chain.
Per shape this measures
  * the device reduction (HIP events inside tci_chainlp: kernel_ms covers the two likelihood launches and the
    tci_chainlp.hip and mean kernels between them; median and range of the repeats; every repeat must give the run's
    own bits),
  * the host route: the device-to-host copy of the chain the reduction avoids (torch, pinned host buffer, HIP
    events), Likelihood.ss_batch on the host chain (wall clock, its own copies included) and the float64 numpy
    restatement (tests/chainlp_oracle.py) of the traces and the reductions,
and checks dev and lp against the long-double restatement in units of the header's bound.
Then fit(TestData, --steps steps, replicates = --replicates, logpost=True) runs once and per cell lp_rhat, ss_gap and
the replicate-pooled standard deviation of ss (the square root of the mean of the replicates' variances of their ss
traces) are recorded: a cell whose ss_gap exceeds that has replicates at visibly different SS levels.
Writes profiles/chainlp/chainlp_time.json.

    python profiles/chainlp/chainlp_time.py [--repeats 11] [--steps 200000] [--long-cells 4] [--replicates 4]
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

import chainlp_oracle as O  # noqa: E402
from transcriptioncycleinference_amd import Likelihood, testdata  # noqa: E402
from transcriptioncycleinference_amd.mcmc import DramOptions, dram_run, fit, plan_fit  # noqa: E402

FIELDS = ("ss", "pri", "dev", "lp") + O.SCALARS + ("best_row", "theta_best", "theta_mean")


def measure(lk, cells, ids, o, repeats, numpy_chains):
    cid = np.array(ids, np.int32)
    p = plan_fit(cells, ids, 0)
    res = dram_run(lk, cid, p.x0, p.lower, p.upper, p.prior_mu, p.prior_sig, p.qcov_diag, 1.0, o, logpost=True)
    k0 = res.chain.shape[0] - res.lp.n_rows
    rows, s2 = np.ascontiguousarray(res.chain[k0:]), np.ascontiguousarray(res.s2chain[k0:])
    n, C, ld = rows.shape
    ms = [res.lp.kernel_ms]
    for _ in range(repeats - 1):
        g = lk.chainlp(rows, s2, cid, p.prior_mu, p.prior_sig)
        ms.append(g.kernel_ms)
        assert all(getattr(g, f).tobytes() == getattr(res.lp, f).tobytes() for f in FIELDS)
    dev = torch.from_numpy(rows).cuda()
    host = torch.empty(rows.shape, dtype=torch.float64).pin_memory()
    copy_ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        host.copy_(dev, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        copy_ms.append(e0.elapsed_time(e1))
    del dev, host
    flat, flat_id = rows.reshape(n * C, ld), np.tile(cid, n)
    lk.ss_batch(flat[:C], flat_id[:C])
    t0 = time.perf_counter()
    ss = lk.ss_batch(flat, flat_id).reshape(n, C)
    ss_batch_s = time.perf_counter() - t0
    assert ss.tobytes() == res.lp.ss.tobytes()
    # the numpy restatement on numpy_chains chains, scaled to all of them
    nc = min(numpy_chains, C)
    P = (7 + cells.lengths[cid]).astype(int)
    nobs = 2.0 * cells.lengths[cid]
    t0 = time.perf_counter()
    pri, dv, lp = O.traces(rows[:, :nc], s2[:, :nc], ss[:, :nc], P[:nc], nobs[:nc], p.prior_mu[:nc], p.prior_sig[:nc])
    tm = np.full((nc, ld), np.nan)
    for c in range(nc):
        tm[c, :P[c]] = O.col_mean(rows[:, c, :P[c]])
    ref = O.reduce({"ss": ss[:, :nc], "pri": pri, "dev": dv, "lp": lp}, s2[:, :nc], rows[:, :nc], P[:nc], nobs[:nc], tm,
                   O.col_mean(s2[:, :nc]), res.lp.ss_hat[:nc])
    numpy_s = time.perf_counter() - t0
    assert np.array_equal(pri, res.lp.pri[:, :nc]) and np.array_equal(ref["best_row"], res.lp.best_row[:nc])
    assert np.array_equal(tm, res.lp.theta_mean[:nc], equal_nan=True)
    e_dev, e_lp = O.bounds(ss[:, :nc], s2[:, :nc], nobs[None, :nc], dv, lp)
    dev_x = O.dev(ss[:, :nc], s2[:, :nc], nobs[None, :nc], exact=True)
    lp_x = O.lp(dev_x, pri, exact=True)
    worst = {"dev": float(np.max(np.abs(res.lp.dev[:, :nc].astype(O.LD) - dev_x).astype(np.float64) / e_dev)),
             "lp": float(np.max(np.abs(res.lp.lp[:, :nc].astype(O.LD) - lp_x).astype(np.float64) / e_lp))}
    med = statistics.median
    return {"rows": n, "n_chains": C, "ld": ld, "chain_bytes": int(rows.nbytes + s2.nbytes), "repeats": len(ms),
            "kernel_ms_median": med(ms), "kernel_ms_min": min(ms), "kernel_ms_max": max(ms),
            "d2h_copy_ms_median": med(copy_ms), "d2h_copy_ms_min": min(copy_ms), "d2h_copy_ms_max": max(copy_ms),
            "host_ss_batch_ms": 1e3 * ss_batch_s, "numpy_chains_timed": nc, "numpy_s_timed": numpy_s,
            "numpy_s_scaled_to_all_chains": numpy_s * C / nc,
            "host_route_ms": med(copy_ms) + 1e3 * ss_batch_s + 1e3 * numpy_s * C / nc,
            "largest_error_over_bound_vs_longdouble": worst, "largest_bound": float(max(np.max(e_dev), np.max(e_lp))),
            "all_chains_finite": bool(np.all(res.lp.best_row >= 0))}


def replicate_finding(lk, steps, thin, M):
    fr = fit(lk, n_steps=steps, n_burn=steps // 2, thin=thin, seed=0, replicates=M, logpost=True)
    cells = []
    for e in fr.MCMClp:
        pooled = float(np.sqrt(np.mean(np.var(e["ss"], axis=1, ddof=1))))
        cells.append({"cell_index": e["cell_index"], "lp_rhat": e["lp_rhat"], "lp_rhat_split": e["lp_rhat_split"],
                      "lp_ess": e["lp_ess"], "ss_gap": e["ss_gap"], "ss_pooled_sd": pooled,
                      "best_replicate": e["best_replicate"]})
    gap = np.array([c["ss_gap"] for c in cells])
    sd = np.array([c["ss_pooled_sd"] for c in cells])
    rh = np.array([c["lp_rhat"] for c in cells])
    return {"steps": steps, "thin": thin, "replicates": M, "rows_per_chain": int(fr.MCMClp[0]["n_rows"]),
            "cells": len(cells), "cells_with_ss_gap_above_pooled_sd": int(np.sum(gap > sd)),
            "cells_with_ss_gap_above_twice_pooled_sd": int(np.sum(gap > 2.0 * sd)),
            "cells_with_lp_rhat_above_1p1": int(np.sum(rh > 1.1)),
            "ss_gap_over_pooled_sd_median": float(np.nanmedian(gap / sd)), "lp_rhat_median": float(np.nanmedian(rh)),
            "sampler_ms": fr.elapsed_ms, "per_cell": cells}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--steps", type=int, default=200000)
    ap.add_argument("--thin", type=int, default=100)
    ap.add_argument("--long-cells", type=int, default=4)
    ap.add_argument("--long-repeats", type=int, default=5)
    ap.add_argument("--replicates", type=int, default=4)
    ap.add_argument("--numpy-chains", type=int, default=32)
    a = ap.parse_args()
    cells = testdata()
    out = {}
    path = os.environ.get("CHAINLP_TIME_JSON") or os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                               "chainlp_time.json")
    with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
        o = DramOptions(n_steps=a.steps, burnintime=a.steps // 2, stats_from=a.steps // 2, thin=a.thin, seed=20201028)
        out["flagship"] = measure(lk, cells, list(range(cells.n_cells)), o, a.repeats, a.numpy_chains)
        print(json.dumps(out["flagship"]), flush=True)
        o = DramOptions(n_steps=a.steps, burnintime=a.steps // 20, stats_from=a.steps // 20, thin=1, seed=20201028)
        ids = [int(c) for c in np.linspace(0, cells.n_cells - 1, a.long_cells).round()]
        out["long_columns"] = measure(lk, cells, ids, o, a.long_repeats, a.long_cells)
        print(json.dumps(out["long_columns"]), flush=True)
        out["testdata_replicates"] = replicate_finding(lk, a.steps, a.thin, a.replicates)
        print(json.dumps({k: v for k, v in out["testdata_replicates"].items() if k != "per_cell"}), flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
