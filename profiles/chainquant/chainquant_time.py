"""Time the posterior-quantile kernel next to what it replaces.

Two cases, each after a TestData fit of 200,000 steps:
  flagship      299 cells, thin = 100: 2,000 kept rows, the post-burn-in 1,000 of them in the quantiles;
  long_columns  a few cells (--long-cells), thin = 1 and stats_from = 10,000: 190,001 rows per column.
For each this measures
  * the selection kernel alone (HIP events around k_cq_select, median and range of the repeats),
  * the device-to-host copy of the same chain rows (torch, pinned host buffer, HIP events),
  * numpy.quantile(method='linear') per chain on the copied rows, theta and s2,
checks the device result bit for bit against the restatement of tests/chainquant_oracle.py (on --oracle-chains
chains of the flagship case, every chain of the long one), and writes profiles/chainquant/chainquant_time.json.

    python profiles/chainquant/chainquant_time.py [--repeats 11] [--steps 200000] [--long-cells 4]
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

import chainquant_oracle as O  # noqa: E402
from transcriptioncycleinference_amd import Likelihood, testdata  # noqa: E402
from transcriptioncycleinference_amd.mcmc import DramOptions, dram_run, plan_fit  # noqa: E402

PROBS = (0.025, 0.5, 0.975)


def measure(lk, cells, ids, o, repeats, oracle_chains):
    p = plan_fit(cells, ids, 0)
    res = dram_run(lk, np.array(ids, np.int32), p.x0, p.lower, p.upper, p.prior_mu, p.prior_sig, p.qcov_diag, 1.0, o,
                   chain_keys=np.array(ids, np.int64), quant=PROBS)
    k0 = res.chain.shape[0] - res.quant.n_rows
    rows, s2 = np.ascontiguousarray(res.chain[k0:]), np.ascontiguousarray(res.s2chain[k0:])
    npar = (7 + cells.lengths[ids]).astype(np.int32)
    ms = [res.quant.kernel_ms]
    for _ in range(max(repeats, 10)):
        cq = lk.chainquant(rows, s2, npar, PROBS)
        ms.append(cq.kernel_ms)
    assert cq.q.tobytes() == res.quant.q.tobytes() and cq.s2_q.tobytes() == res.quant.s2_q.tobytes()
    # the copy the device reduction makes unnecessary
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
    n, nch, ld = rows.shape
    # the host reduction of the copied chain
    t0 = time.perf_counter()
    for c in range(nch):
        np.quantile(rows[:, c, :npar[c]], PROBS, axis=0, method="linear")
        np.quantile(s2[:, c], PROBS, method="linear")
    numpy_s = time.perf_counter() - t0
    noc = nch if oracle_chains <= 0 else min(oracle_chains, nch)
    want = O.table(rows[:, :noc], s2[:, :noc], npar[:noc], PROBS)
    assert res.quant.q[:noc].tobytes() == want["q"].tobytes() and res.quant.s2_q[:noc].tobytes() == want["s2_q"].tobytes()
    kernel = statistics.median(ms)
    return {
        "rows": n, "n_chains": nch, "ld": ld, "probs": list(PROBS), "chain_bytes": int(rows.nbytes + s2.nbytes),
        "columns": int(npar.sum()) + nch, "fit_elapsed_ms": res.elapsed_ms,
        "kernel_ms_median": kernel, "kernel_ms_min": min(ms), "kernel_ms_max": max(ms), "repeats": len(ms),
        "d2h_copy_ms_median": statistics.median(copy_ms),
        "numpy_quantile_s": numpy_s,
        "host_route_ms": statistics.median(copy_ms) + 1e3 * numpy_s,
        "kernel_beats_host_route": bool(kernel < statistics.median(copy_ms) + 1e3 * numpy_s),
        "bitwise_equal_to_the_restatement_on_chains": noc,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--steps", type=int, default=200000)
    ap.add_argument("--thin", type=int, default=100)
    ap.add_argument("--long-cells", type=int, default=4)
    ap.add_argument("--oracle-chains", type=int, default=16)
    a = ap.parse_args()
    cells = testdata()
    out = {}
    with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
        o = DramOptions(n_steps=a.steps, burnintime=a.steps // 2, stats_from=a.steps // 2, thin=a.thin, seed=20201028)
        out["flagship"] = measure(lk, cells, list(range(cells.n_cells)), o, a.repeats, a.oracle_chains)
        print(json.dumps(out["flagship"]), flush=True)
        o = DramOptions(n_steps=a.steps, burnintime=a.steps // 20, stats_from=a.steps // 20, thin=1, seed=20201028)
        ids = [int(c) for c in np.linspace(0, cells.n_cells - 1, a.long_cells).round()]
        out["long_columns"] = measure(lk, cells, ids, o, a.repeats, 0)
        print(json.dumps(out["long_columns"]), flush=True)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "chainquant_time.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
