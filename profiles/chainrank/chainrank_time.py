"""Time the rank diagnostics (tci_chainrank) next to tci_chainess on the same chains and next to the host route.

Three cases:
  flagship      299 cells x --replicates chains, --steps steps, thinned so that 1,000 kept rows past burn-in enter the
                reduction (N = 4,000 per group: the LDS sort), max_lag = 0;
  long_columns  --long-cells cells, thin = 1, stats_from = steps / 20 of --long-steps steps (the 190,000 rows from kept
                row steps / 20 on, N = 760,000 per group: the global-memory sort), max_lag = --long-max-lag;
  demc          299 cells x 64 members x 101 kept rows of a DE-MC run (N = 6,464: the LDS sort).
For each: the device time of the whole reduction and of the sort / rank / indicator kernels alone (HIP events, median
and range over the repeats), tci_chainess on the same chains, and for the flagship the device-to-host copy of the rows
plus the numpy restatement (tests/chainrank_oracle.py) on --host-groups groups, scaled to all. The flagship also gives
the findings on TestData: rhat_rank against the classic R-hat per cell, the cells whose folded R-hat exceeds the bulk
one, ess_tail against ess_bulk, and the pooled 2.5 / 50 / 97.5 % of v against replicate 0's.

    python profiles/chainrank/chainrank_time.py [--out profiles/chainrank/chainrank_time.json]
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

import chainrank_oracle as O  # noqa: E402
from transcriptioncycleinference_amd import Likelihood, mcmc, testdata  # noqa: E402
from transcriptioncycleinference_amd.mcmc import DramOptions, dram_run, plan_fit, replicate_keys  # noqa: E402


def spread(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "repeats": len(ms)}


def time_reductions(lk, rows, s2, npar, group, max_lag, repeats):
    whole, rank, ess = [], [], []
    first = None
    for _ in range(repeats):
        ck = lk.chainrank(rows, s2, npar, group, max_lag=max_lag)
        whole.append(ck.kernel_ms)
        rank.append(ck.rank_ms)
        ess.append(lk.chainess(rows, s2, npar, group, max_lag=max_lag).kernel_ms)
        first = first or ck
    n, nch, ld = rows.shape
    return first, {"rows": n, "n_chains": nch, "ld": ld, "max_lag": max_lag, "values_per_group": int(n * np.sum(group == 0)),
                   "chain_bytes": int(rows.nbytes + s2.nbytes), "chainrank_ms": spread(whole), "rank_kernels_ms": spread(rank),
                   "rank_kernels_share": statistics.median(rank) / statistics.median(whole), "chainess_ms": spread(ess)}


def host_route(rows, s2, npar, group, K, host_groups, repeats):
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
    ng = min(host_groups, K)
    sel = np.nonzero(group < ng)[0]
    t0 = time.perf_counter()
    O.table(rows[:, sel], s2[:, sel], npar[sel], group[sel])
    numpy_s = time.perf_counter() - t0
    return {"d2h_copy_ms": spread(copy_ms), "numpy_groups": ng, "numpy_s_those_groups": numpy_s,
            "numpy_s_scaled_to_all_groups": numpy_s * K / ng}


def findings(lk, ck, rows, s2, npar, group, K):
    """What the rank diagnostics say on TestData, per cell over its real columns (theta and s2)."""
    ld = rows.shape[2]
    real = np.arange(ld)[None, :] < npar[:K, None]
    cr = lk.chainrhat(rows, s2, npar, group)
    m = lambda a: np.nanmax(np.where(real, a, np.nan), axis=1)  # noqa: E731
    rank_max, classic_max, bulk_max, folded_max = m(ck.rhat_rank), m(cr.rhat), m(ck.rhat_bulk), m(ck.rhat_folded)
    med = lambda a: float(np.nanmedian(np.where(real, a, np.nan)))  # noqa: E731
    rep0 = lk.chainquant(rows[:, :K], s2[:, :K], npar[:K])
    v = mcmc.THETA_INDEX["v"]
    return {"cells": K, "largest_rhat_rank_per_cell_median": float(np.median(rank_max)),
            "largest_classic_rhat_per_cell_median": float(np.median(classic_max)),
            "cells_rhat_rank_above_classic": int(np.sum(rank_max > classic_max)),
            "cells_rhat_rank_above_1p01": int(np.sum(rank_max > 1.01)),
            "cells_folded_above_bulk": int(np.sum(folded_max > bulk_max)),
            "columns_folded_above_bulk": int(np.sum(np.where(real, ck.rhat_folded > ck.rhat_bulk, False))),
            "columns": int(real.sum()), "ess_bulk_median": med(ck.ess_bulk), "ess_tail_median": med(ck.ess_tail),
            "ess_classic_split_median": med(lk.chainess(rows, s2, npar, group).ess_split),
            "v_pooled_q_median_over_cells": [float(x) for x in np.median(ck.q[:, :, v], axis=0)],
            "v_replicate0_q_median_over_cells": [float(x) for x in np.median(rep0.q[:, :, v], axis=0)],
            "v_pooled_interval_over_replicate0_interval_median":
                float(np.median((ck.q[:, 2, v] - ck.q[:, 0, v]) / (rep0.q[:, 2, v] - rep0.q[:, 0, v])))}


def dram_rows(lk, cells, ids, o, M):
    K = len(ids)
    group = np.tile(np.arange(K, dtype=np.int32), M)
    p = plan_fit(cells, ids, 0, replicates=M)
    res = dram_run(lk, np.tile(np.array(ids, np.int32), M), p.x0, p.lower, p.upper, p.prior_mu, p.prior_sig, p.qcov_diag,
                   1.0, o, chain_keys=replicate_keys(ids, M))
    k0 = (o.stats_from + o.thin - 1) // o.thin
    npar = (7 + cells.lengths[np.tile(ids, M)]).astype(np.int32)
    return np.ascontiguousarray(res.chain[k0:]), np.ascontiguousarray(res.s2chain[k0:]), npar, group


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--thin", type=int, default=10)
    ap.add_argument("--long-steps", type=int, default=200000)
    ap.add_argument("--long-cells", type=int, default=4)
    ap.add_argument("--long-max-lag", type=int, default=2000)
    ap.add_argument("--long-repeats", type=int, default=2)
    ap.add_argument("--replicates", type=int, default=4)
    ap.add_argument("--host-groups", type=int, default=8)
    ap.add_argument("--demc-gen", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "chainrank_time.json"))
    a = ap.parse_args()
    cells = testdata()
    out = {"lds_cap": None}
    with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
        out["lds_cap"] = int(lk._lib.tci_chainrank_lds_cap())
        ids = list(range(cells.n_cells))
        o = DramOptions(n_steps=a.steps, burnintime=a.steps // 2, stats_from=a.steps // 2, thin=a.thin, seed=20201028)
        rows, s2, npar, group = dram_rows(lk, cells, ids, o, a.replicates)
        ck, out["flagship"] = time_reductions(lk, rows, s2, npar, group, 0, a.repeats)
        out["flagship"].update(host_route(rows, s2, npar, group, len(ids), a.host_groups, a.repeats))
        out["flagship"]["findings"] = findings(lk, ck, rows, s2, npar, group, len(ids))
        print(json.dumps(out["flagship"]), flush=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)

        sp = mcmc.search_population(cells, ids, 20201028, 64)
        jit = np.zeros_like(sp.lower)
        j = mcmc.demc_jitter(cells, sp.cells)
        jit[:, :j.shape[1]] = j
        dm = lk.demc(sp.pop0, np.array(sp.cells, np.int32), sp.lower, sp.upper, sp.prior_mu, sp.prior_sig, jit,
                     seed=20201028, n_gen=a.demc_gen, thin=1)
        P = (7 + cells.lengths[np.array(sp.cells)]).astype(np.int32)
        _, out["demc"] = time_reductions(lk, dm.chain, dm.s2chain, np.repeat(P, 64),
                                         np.repeat(np.arange(len(ids), dtype=np.int32), 64), 0, a.repeats)
        print(json.dumps(out["demc"]), flush=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)

        o = DramOptions(n_steps=a.long_steps, burnintime=a.long_steps // 20, stats_from=a.long_steps // 20, thin=1,
                        seed=20201028)
        lids = [int(c) for c in np.linspace(0, cells.n_cells - 1, a.long_cells).round()]
        rows, s2, npar, group = dram_rows(lk, cells, lids, o, a.replicates)
        _, out["long_columns"] = time_reductions(lk, rows, s2, npar, group, a.long_max_lag, a.long_repeats)
        print(json.dumps(out["long_columns"]), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
