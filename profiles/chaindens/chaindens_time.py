"""Time the marginal-density kernels next to what they replace.

Two cases, each after a TestData fit of 200,000 steps:
  flagship      299 cells, thin = 100: 2,000 kept rows, the post-burn-in 1,000 of them in the densities;
  long_columns  a few cells (--long-cells), thin = 1 and stats_from = 10,000: 190,001 rows per column.
For each this measures
  * the kernels alone (HIP events around launch_chaindens, the quartile selection included; median and range of
    the repeats after a warm-up call),
  * the device-to-host copy of the same chain rows (torch, pinned host buffer, HIP events),
  * the numpy restatement of tests/chaindens_oracle.py on the copied rows (on --oracle-chains chains, scaled to all
    of them) and scipy's gaussian_kde plus numpy.histogram on the same chains, if scipy imports,
checks the device result against the restatement within the bounds derived there (range, grid and counts bit for
bit), and writes profiles/chaindens/chaindens_time.json.

    python profiles/chaindens/chaindens_time.py [--repeats 11] [--steps 200000] [--long-cells 4]
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

import chaindens_oracle as O  # noqa: E402
from transcriptioncycleinference_amd import Likelihood, testdata  # noqa: E402
from transcriptioncycleinference_amd.mcmc import DramOptions, dram_run, plan_fit  # noqa: E402


def measure(lk, cells, ids, o, repeats, oracle_chains):
    p = plan_fit(cells, ids, 0)
    res = dram_run(lk, np.array(ids, np.int32), p.x0, p.lower, p.upper, p.prior_mu, p.prior_sig, p.qcov_diag, 1.0, o,
                   chain_keys=np.array(ids, np.int64), dens=True)
    k0 = res.chain.shape[0] - res.dens.n_rows
    rows, s2 = np.ascontiguousarray(res.chain[k0:]), np.ascontiguousarray(res.s2chain[k0:])
    npar = (7 + cells.lengths[ids]).astype(np.int32)
    lk.chaindens(rows, s2, npar)                       # warm-up of the host-chain path
    ms = []
    for _ in range(max(repeats, 10)):
        cd = lk.chaindens(rows, s2, npar)
        ms.append(cd.kernel_ms)
    assert all(getattr(cd, k).tobytes() == getattr(res.dens, k).tobytes()
               for k in ("range", "bw", "dens", "counts", "s2_dens", "s2_counts"))
    # the copy the device reduction makes unnecessary
    dev = torch.from_numpy(rows).cuda()
    host = torch.empty(rows.shape, dtype=torch.float64).pin_memory()
    copy_ms = []
    for _ in range(max(repeats, 10) + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        host.copy_(dev, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        copy_ms.append(e0.elapsed_time(e1))
    copy_ms = copy_ms[1:]                              # the first copy warms up
    del dev, host
    n, nch, ld = rows.shape
    # the host reduction of the copied chain, on noc chains and scaled to all of them by their columns
    noc = nch if oracle_chains <= 0 else min(oracle_chains, nch)
    t0 = time.perf_counter()
    want = O.table(rows[:, :noc], s2[:, :noc], npar[:noc])
    oracle_s = time.perf_counter() - t0
    sub = type(res.dens)(*[getattr(res.dens, k)[:noc] for k in ("range", "bw", "dens", "counts", "s2_range", "s2_bw",
                                                                 "s2_dens", "s2_counts")])
    worst = O.compare(sub, want, n, "profile")
    cols_all, cols_sub = int(npar.sum()) + nch, int(npar[:noc].sum()) + noc
    numpy_s = oracle_s * cols_all / cols_sub
    kde_s = None
    try:
        from scipy.stats import gaussian_kde

        t0 = time.perf_counter()
        for c in range(noc):
            for x in [rows[:, c, j] for j in range(int(npar[c]))] + [s2[:, c]]:
                if x.min() < x.max():
                    g = O.grid_of(x.min(), x.max(), 100)
                    gaussian_kde(x)(g)
                    np.histogram(x, 20)
        kde_s = (time.perf_counter() - t0) * cols_all / cols_sub
    except ImportError:
        pass
    kernel, copy = statistics.median(ms), statistics.median(copy_ms)
    host_s = numpy_s if kde_s is None else min(numpy_s, kde_s)
    return {
        "rows": n, "n_chains": nch, "ld": ld, "n_grid": 100, "n_bins": 20, "chain_bytes": int(rows.nbytes + s2.nbytes),
        "columns": cols_all, "exp_evaluations": int(cols_all) * n * 100, "fit_elapsed_ms": res.elapsed_ms,
        "kernel_ms_median": kernel, "kernel_ms_min": min(ms), "kernel_ms_max": max(ms), "repeats": len(ms),
        "kernel_ms_inside_the_fit": res.dens.kernel_ms,
        "gexp_per_s": int(cols_all) * n * 100 / kernel / 1e6,
        "d2h_copy_ms_median": copy,
        "numpy_restatement_s": numpy_s, "scipy_gaussian_kde_s": kde_s, "host_timed_on_chains": noc,
        "host_route_ms": copy + 1e3 * host_s,
        "kernel_beats_host_route": bool(kernel < copy + 1e3 * host_s),
        "kernel_beats_the_copy_alone": bool(kernel < copy),
        "checked_against_the_restatement_on_chains": noc, "worst_bw_and_dens_error_over_bound": worst,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--steps", type=int, default=200000)
    ap.add_argument("--thin", type=int, default=100)
    ap.add_argument("--long-cells", type=int, default=4)
    ap.add_argument("--oracle-chains", type=int, default=8)
    ap.add_argument("--long-oracle-chains", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "chaindens_time.json"))
    a = ap.parse_args()
    cells = testdata()
    out = {}
    with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
        o = DramOptions(n_steps=a.steps, burnintime=a.steps // 2, stats_from=a.steps // 2, thin=a.thin, seed=20201028)
        out["flagship"] = measure(lk, cells, list(range(cells.n_cells)), o, a.repeats, a.oracle_chains)
        print(json.dumps(out["flagship"]), flush=True)
        o = DramOptions(n_steps=a.steps, burnintime=a.steps // 20, stats_from=a.steps // 20, thin=1, seed=20201028)
        ids = [int(c) for c in np.linspace(0, cells.n_cells - 1, a.long_cells).round()]
        out["long_columns"] = measure(lk, cells, ids, o, a.repeats, a.long_oracle_chains)
        print(json.dumps(out["long_columns"]), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
