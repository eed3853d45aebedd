"""Time PSIS-LOO with stacking next to what it replaces, and measure how the stacking weights distribute on TestData.

Timing workload: the 299 TestData cells x --replicates (4) chains x --samples (500) samples drawn around each cell's
fixture chain state (every replicate its own draws), sigma2 = 1, the replicates of a cell as one group. This measures
  * the loocheck kernel and the forward launch that fills its scratch (HIP events inside tci_loocheck: kernel_ms and
    forward_ms; median and range of the repeats), and the wall time of the whole call (host stacking included),
  * the device-to-host copy of the simulated rows the reduction avoids (2 x 1196 x S x N_max doubles; torch, pinned
    host buffer, HIP events, in as many pieces as the scratch has chunks),
  * the numpy restatement (tests/loocheck_oracle.py, float64 path) on those rows, timed on --oracle-cells chains and
    scaled to all of them,
and checks the device result against that restatement on the same chains.

Weights: fit(..., replicates=4, stack=--samples) of all 299 cells with --fit-steps steps (half of them burn-in, every
--fit-thin-th row kept): the distribution of the largest weight of a cell, of the Pareto k and of elpd_stack against the
best single replicate.

Writes profiles/loocheck/loocheck_time.json with the commit it ran on.

    python profiles/loocheck/loocheck_time.py [--repeats 7] [--samples 500] [--oracle-cells 4] [--fit-steps 20000]

profiles/loocheck/tolerance.json is a record of another kind: the float64 / long-double differences the GPU tests
measure on their own inputs. Regenerate it with
    TCI_LOOCHECK_TOLERANCE_LOG=log.jsonl python -m pytest tests/test_loocheck_gpu.py
    python profiles/loocheck/loocheck_time.py --tolerance-log log.jsonl
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import loocheck_oracle as LO  # noqa: E402
from transcriptioncycleinference_amd import Likelihood, mcmc, testdata  # noqa: E402


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return "unknown"


def tolerance_record(log):
    rows = [json.loads(line) for line in open(log)]
    largest = {}
    for r in rows:
        for k, v in r.items():
            if k != "case":
                largest[k] = max(largest.get(k, 0.0), v)
    out = {"what": "largest |float64 restatement - numpy.longdouble restatement| (tests/loocheck_oracle.py) on the inputs "
                   "of tests/test_loocheck_gpu.py, per call; each test measures the difference on its call's own inputs "
                   "and allows factor x that call's value",
           "regenerate": "TCI_LOOCHECK_TOLERANCE_LOG=log.jsonl python -m pytest tests/test_loocheck_gpu.py; "
                         "python profiles/loocheck/loocheck_time.py --tolerance-log log.jsonl",
           "factor": 8.0, "largest": largest, "per_call": rows}
    with open(os.path.join(HERE, "tolerance.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def weights(lk, a):
    t0 = time.perf_counter()
    fit = mcmc.fit(lk, n_steps=a.fit_steps, n_burn=a.fit_steps // 2, seed=0, thin=a.fit_thin, replicates=a.replicates,
                   stack=a.samples)
    wall = time.perf_counter() - t0
    st = fit.MCMCstack
    w = np.stack([e["weights"] for e in st])
    top = w.max(axis=1)
    gain = np.array([e["elpd_stack"] - np.max(e["elpd_loo"]) for e in st])
    bad = np.stack([e["n_khat_bad"] for e in st])
    kmax = np.stack([e["khat_max"] for e in st])
    rmax = np.array([e["rhat_max"] for e in fit.MCMCrhat])
    share = lambda m: float(np.mean(m))  # noqa: E731
    return {"n_steps": a.fit_steps, "n_burn": a.fit_steps // 2, "thin": a.fit_thin, "replicates": a.replicates,
            "samples": int(st[0]["n_samples"]), "cells": len(st), "fit_wall_s": wall,
            "share_top_weight_above_0.9": share(top > 0.9), "share_top_weight_above_0.99": share(top > 0.99),
            "share_top_weight_below_0.5": share(top < 0.5), "top_weight_median": float(np.median(top)),
            "top_weight_quartiles": np.quantile(top, [0.25, 0.5, 0.75]).tolist(),
            "share_replicates_with_weight_below_0.01": share(w < 0.01),
            "share_cells_top_weight_is_best_elpd_loo": share(w.argmax(axis=1) == np.stack(
                [e["elpd_loo"] for e in st]).argmax(axis=1)),
            "elpd_stack_minus_best_elpd_loo_median": float(np.median(gain)),
            "elpd_stack_minus_best_elpd_loo_max": float(np.max(gain)),
            "share_chains_with_a_khat_above_threshold": share(bad > 0),
            "points_above_threshold_per_chain_median": float(np.median(bad)),
            "share_chains_with_degenerate_tail": share(np.isinf(kmax)),
            "khat_max_median_of_finite": float(np.median(kmax[np.isfinite(kmax)])) if np.isfinite(kmax).any() else None,
            "share_cells_rhat_max_above_1.1": share(rmax > 1.1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--samples", type=int, default=500)
    ap.add_argument("--replicates", type=int, default=4)
    ap.add_argument("--oracle-cells", type=int, default=4)
    ap.add_argument("--fit-steps", type=int, default=20000, help="0: skip the weights")
    ap.add_argument("--fit-thin", type=int, default=10)
    ap.add_argument("--tolerance-log", default=None, help="only rewrite tolerance.json from this log of the GPU tests")
    ap.add_argument("--commit", default=None, help="the commit the tree was taken from (default: git rev-parse HEAD)")
    a = ap.parse_args()
    if a.tolerance_log:
        return tolerance_record(a.tolerance_log)
    cells = testdata()
    S, K, R = a.samples, cells.n_cells, a.replicates
    with np.load(os.path.join(ROOT, "tests", "golden", "chain_theta.npz"), allow_pickle=False) as f:
        z = {k: f[k] for k in f.files}
    off, pick = z["theta_offsets"], np.nonzero(z["step"] == 9)[0]   # the last fixture chain row of every cell
    ld = 7 + int(cells.lengths.max())
    rng = np.random.default_rng(20201028)
    theta = np.zeros((R * K, S, ld))
    cid = np.tile(z["cell_id"][pick].astype(np.int32), R)
    for r in range(R):
        for k, i in enumerate(pick):
            row = z["theta"][off[i]:off[i + 1]]
            theta[r * K + k, :, :len(row)] = row[None, :] * (1.0 + 0.01 * rng.normal(size=(S, len(row))))
    s2 = np.ones((R * K, S))
    group = np.tile(np.arange(K, dtype=np.int32), R)
    with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
        lk.loocheck(theta[:2], s2[:2], cid[:2])                           # warm-up: code objects
        kern, fwd, wall = [], [], []
        for _ in range(max(a.repeats, 3)):
            t0 = time.perf_counter()
            lc = lk.loocheck(theta, s2, cid, group=group)
            wall.append(1e3 * (time.perf_counter() - t0))
            kern.append(lc.kernel_ms)
            fwd.append(lc.forward_ms)
        n_max = lc.khat_i.shape[2]
        sim_bytes = 2 * R * K * S * n_max * 8
        pieces = -(-sim_bytes // (1 << 30))
        dev = torch.empty(sim_bytes // 8 // pieces, dtype=torch.float64, device="cuda")
        host = torch.empty(sim_bytes // 8 // pieces, dtype=torch.float64).pin_memory()
        copy_ms = []
        for _ in range(max(a.repeats, 3)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(pieces):
                host.copy_(dev, non_blocking=True)
            e1.record()
            torch.cuda.synchronize()
            copy_ms.append(e0.elapsed_time(e1))
        del dev, host
        nc = min(a.oracle_cells, R * K)
        ms2, pp7 = lk.forward(theta[:nc].reshape(nc * S, ld), np.repeat(cid[:nc], S), grid="interp")
        stacking = weights(lk, a) if a.fit_steps > 0 else None
    numpy_s, worst = 0.0, {"elpd_loo_i": 0.0, "p_loo_i": 0.0, "khat_i": 0.0}
    for k in range(nc):
        _, y0, y1 = cells.cell(int(cid[k]))
        n = len(y0)
        m, p = ms2[k * S:(k + 1) * S, :n], pp7[k * S:(k + 1) * S, :n]
        t0 = time.perf_counter()
        ref = LO.chain(m, p, y0, y1, s2[k])
        numpy_s += time.perf_counter() - t0
        fin = np.isfinite(ref["khat_i"])
        assert np.array_equal(np.isposinf(lc.khat_i[k][:, :n]), np.isposinf(ref["khat_i"]))
        assert np.array_equal(np.isnan(lc.khat_i[k][:, :n]), np.isnan(ref["khat_i"]))
        for f in worst:
            if fin.any():
                worst[f] = max(worst[f], float(np.max(np.abs(getattr(lc, f)[k][:, :n][fin] - ref[f][fin]))))
    med = statistics.median
    M, G = LO.tail_count(S)
    out = {
        "commit": a.commit or commit(), "cells": K, "replicates": R, "chains": R * K, "samples": S, "tail_M": M,
        "profile_G": G, "n_max": int(n_max), "sim_bytes_avoided": sim_bytes, "repeats": len(kern),
        "lds_bytes_per_workgroup": 64 * (10 * M + 8 * G),
        "loocheck_kernel_ms_median": med(kern), "loocheck_kernel_ms_min": min(kern), "loocheck_kernel_ms_max": max(kern),
        "forward_ms_median": med(fwd), "forward_ms_min": min(fwd), "forward_ms_max": max(fwd),
        "call_wall_ms_median": med(wall), "call_wall_ms_min": min(wall), "call_wall_ms_max": max(wall),
        "d2h_copy_ms_median": med(copy_ms), "d2h_copy_ms_min": min(copy_ms), "d2h_copy_ms_max": max(copy_ms),
        "numpy_chains_timed": nc, "numpy_s_timed": numpy_s, "numpy_s_scaled_to_all_chains": numpy_s * R * K / nc,
        "largest_difference_from_float64_restatement": worst,
        "stacking_iterations_median": float(np.median(lc.n_iter)), "stacking_iterations_max": int(np.max(lc.n_iter)),
        "stacking_on_testdata": stacking,
    }
    print(json.dumps(out), flush=True)
    path = os.environ.get("LOOCHECK_TIME_JSON") or os.path.join(HERE, "loocheck_time.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
