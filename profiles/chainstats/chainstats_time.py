"""Time the chain-diagnostics kernels next to what they replace.

After a TestData fit of 299 cells x 200,000 steps with thin = 100 (2,000 kept rows, the post-burn-in
half of them in the statistics) this measures
  * the statistics kernels alone (HIP events around k_cs_moments + k_cs_iact, median of the repeats),
  * the device-to-host copy of the same chain rows (torch, pinned host buffer, HIP events),
  * the numpy oracle of tests/chainstats_oracle.py on the host,
and writes profiles/chainstats/chainstats_time.json.

    python profiles/chainstats/chainstats_time.py [--repeats 11] [--steps 200000]
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

import chainstats_oracle as O  # noqa: E402
from transcriptioncycleinference_amd import Likelihood, testdata  # noqa: E402
from transcriptioncycleinference_amd.mcmc import DramOptions, dram_run, plan_fit  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--steps", type=int, default=200000)
    ap.add_argument("--thin", type=int, default=100)
    a = ap.parse_args()
    cells = testdata()
    ids = list(range(cells.n_cells))
    with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
        p = plan_fit(cells, ids, 0)
        o = DramOptions(n_steps=a.steps, burnintime=a.steps // 2, stats_from=a.steps // 2, thin=a.thin, seed=20201028)
        res = dram_run(lk, np.array(ids, np.int32), p.x0, p.lower, p.upper, p.prior_mu, p.prior_sig, p.qcov_diag, 1.0,
                       o, chain_keys=np.array(ids, np.int64), stats=True)
        k0 = res.chain.shape[0] - res.stats.n_rows
        rows, s2 = np.ascontiguousarray(res.chain[k0:]), np.ascontiguousarray(res.s2chain[k0:])
        npar = (7 + cells.lengths[ids]).astype(np.int32)
        ms = [res.stats.kernel_ms]
        for _ in range(max(a.repeats, 10)):
            st = lk.chainstats(rows, s2, npar)
            ms.append(st.kernel_ms)
        assert st.tau.tobytes() == res.stats.tau.tobytes()
    # the copy the statistics make unnecessary
    dev = torch.from_numpy(rows).cuda()
    host = torch.empty(rows.shape, dtype=torch.float64).pin_memory()
    copy_ms = []
    for _ in range(max(a.repeats, 10)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        host.copy_(dev, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        copy_ms.append(e0.elapsed_time(e1))
    t0 = time.perf_counter()
    want = O.table(rows, s2, npar)
    oracle_s = time.perf_counter() - t0
    n, nch, ld = rows.shape
    win = res.stats.tau_window
    lag_tiles = int(np.ceil(max(int(win.max()), 1) / 64))
    out = {
        "rows": n, "n_chains": nch, "ld": ld, "chain_bytes": int(rows.nbytes),
        "fit_elapsed_ms": res.elapsed_ms,
        "stats_kernels_ms_median": statistics.median(ms), "stats_kernels_ms_min": min(ms), "stats_kernels_ms_max": max(ms),
        "repeats": len(ms),
        "d2h_copy_ms_median": statistics.median(copy_ms),
        "numpy_oracle_s": oracle_s,
        "tau_window_max": int(win.max()), "tau_window_median": float(np.median(win[win >= 0])),
        "lag_tiles_of_the_slowest_column": lag_tiles,
        "algorithmic_bytes_upper": int(8 * n * nch * ld * (1 + lag_tiles)),
        "oracle_margin": want["margin"],
        "tau_max_rel_err": O.rel_err(res.stats.tau, want["tau"]) if want["margin"] >= 1e-6 else None,
    }
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "chainstats_time.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
