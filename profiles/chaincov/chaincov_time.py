"""Time the posterior-covariance kernels next to what they replace.

After a TestData fit of 299 cells x 200,000 steps with thin = 100 (2,000 kept rows, the post-burn-in
half of them in the matrices) this measures
  * the covariance kernels alone (HIP events around k_cc_mean + k_cc_cov + k_cc_corr, median of the repeats),
  * the device-to-host copy of the same chain rows (torch, pinned host buffer, HIP events),
  * the host reduction of the copied chain: numpy's cov / corrcoef per chain in FP64, and the longdouble
    restatement of tests/chaincov_oracle.py (on --oracle-chains chains; 0 = all of them),
and writes profiles/chaincov/chaincov_time.json.

    python profiles/chaincov/chaincov_time.py [--repeats 11] [--steps 200000] [--oracle-chains 0]
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

import chaincov_oracle as O  # noqa: E402
from transcriptioncycleinference_amd import Likelihood, testdata  # noqa: E402
from transcriptioncycleinference_amd.mcmc import DramOptions, dram_run, plan_fit  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--steps", type=int, default=200000)
    ap.add_argument("--thin", type=int, default=100)
    ap.add_argument("--oracle-chains", type=int, default=0)
    a = ap.parse_args()
    cells = testdata()
    ids = list(range(cells.n_cells))
    with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
        p = plan_fit(cells, ids, 0)
        o = DramOptions(n_steps=a.steps, burnintime=a.steps // 2, stats_from=a.steps // 2, thin=a.thin, seed=20201028)
        res = dram_run(lk, np.array(ids, np.int32), p.x0, p.lower, p.upper, p.prior_mu, p.prior_sig, p.qcov_diag, 1.0,
                       o, chain_keys=np.array(ids, np.int64), cov=True)
        k0 = res.chain.shape[0] - res.cov.n_rows
        rows = np.ascontiguousarray(res.chain[k0:])
        npar = (7 + cells.lengths[ids]).astype(np.int32)
        ms = [res.cov.kernel_ms]
        for _ in range(max(a.repeats, 10)):
            cc = lk.chaincov(rows, npar)
            ms.append(cc.kernel_ms)
        assert cc.cov.tobytes() == res.cov.cov.tobytes() and cc.corr.tobytes() == res.cov.corr.tobytes()
    # the copy the device reduction makes unnecessary
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
    n, nch, ld = rows.shape
    # the host reduction of the copied chain, FP64
    t0 = time.perf_counter()
    for c in range(nch):
        x = rows[:, c, :npar[c]]
        np.cov(x, rowvar=False, ddof=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            np.corrcoef(x, rowvar=False)
    numpy_s = time.perf_counter() - t0
    # ... and the longdouble restatement, which is also the accuracy check
    noc = nch if a.oracle_chains <= 0 else min(a.oracle_chains, nch)
    t0 = time.perf_counter()
    want = O.table(rows[:, :noc], npar[:noc])
    oracle_s = time.perf_counter() - t0

    class Sub:
        mean, cov, corr = res.cov.mean[:noc], res.cov.cov[:noc], res.cov.corr[:noc]

    worst = O.check(Sub, want, n, "chaincov_time ")
    out = {
        "rows": n, "n_chains": nch, "ld": ld, "chain_bytes": int(rows.nbytes),
        "matrix_bytes": int(res.cov.cov.nbytes + res.cov.corr.nbytes),
        "fit_elapsed_ms": res.elapsed_ms,
        "cov_kernels_ms_median": statistics.median(ms), "cov_kernels_ms_min": min(ms), "cov_kernels_ms_max": max(ms),
        "repeats": len(ms),
        "d2h_copy_ms_median": statistics.median(copy_ms),
        "numpy_fp64_cov_corrcoef_s": numpy_s,
        "restatement_chains": noc, "restatement_s": oracle_s,
        "mfma_flops": int(sum(2 * n * ((int(P) + 15) // 16 * 16) ** 2 // 2 for P in npar)),
        "algorithmic_bytes": int(8 * n * int(npar.sum())),
        "errors_in_units_of_the_bound": worst,
    }
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "chaincov_time.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
