"""Time the DE-MC population sampler on TestData against its floor and summarise what it samples.

    python profiles/demc/demc_time.py [--pop 64] [--gens 2000] [--thin 10] [--out profiles/demc/demc_time.json]
    rocprofv3 --kernel-trace --stats -d DIR -o demc -- python profiles/demc/demc_time.py --trace-only
    python profiles/demc/demc_time.py --kernel-stats DIR/.../demc_kernel_stats.csv   (merges the split into --out)

(a) device time (HIP events, one run after a small warm-up run) of mcmc.demc on all cells against the same number of bare
likelihood launches on the same row counts in the same process: one launch of n_cells * n_pop rows for generation 0 and,
per generation, one of n_cells * ceil(n_pop / 2) and one of n_cells * floor(n_pop / 2) rows.
(b) per cell: the largest classic R-hat and the least multi-chain ESS across the members, the mean SS of the kept rows
past burn-in, the accept rate and the share of proposals rejected at the bounds, beside the same figures of the
four-replicate DRAM fit and its tempered and presearched variants, read from profiles/temper/temper_time.json and
profiles/modesearch/modesearch_time.json as they stand (not re-derived). One run each; no spread is quoted.
--trace-only runs the sampler alone (the warm-up's small launches included), for one kernel trace in a process of its
own; --kernel-stats reads that trace's per-kernel statistics and adds the split between the three kernels to the JSON."""
import csv
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # the HIP runtime before libtci.so, as bench.py loads it

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))


def floor_ms(lk, rows, cid, launches):
    th = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    c = torch.from_numpy(np.ascontiguousarray(cid)).cuda()
    out = torch.empty(len(cid), dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream()
    lk.ss_batch_device(th, c, out, stream=st)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        lk.ss_batch_device(th, c, out, stream=st)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


HERE = os.path.dirname(os.path.abspath(__file__))


def comparison():
    """The parent's figures, [5th, 50th, 95th percentile] over the cells where they are lists."""
    t = json.load(open(os.path.join(HERE, "..", "temper", "temper_time.json")))
    m = json.load(open(os.path.join(HERE, "..", "modesearch", "modesearch_time.json")))
    row = lambda d, ss, ms: dict(rhat_max_p5_p50_p95=d["rhat_max"], cells_rhat_above_1p1=d["rhat_max_above_1p1"],  # noqa: E731
                                 ess_min_p5_p50_p95=d.get("ess_min"), mean_ss_p5_p50_p95=d[ss], device_ms=ms)
    return dict(source="profiles/temper/temper_time.json, profiles/modesearch/modesearch_time.json; 4 replicates, "
                       "20,000 steps, every 10th row kept; mean_ss of the DRAM rows is the best replicate's; accept rate "
                       "and out-of-bounds share are not in those files",
                dram_4_replicates=row(t["plain_replicates"], "ss_mean", t["plain"]["device_ms"]),
                tempered_4_rungs=row(t["cold_rungs"], "ss_mean", t["tempered"]["device_ms"]),
                presearched=row(m["presearch_fit"], "best_replicate_ss_mean", m["presearch_fit"]["device_ms"]))


def kernel_split(path):
    """Per kernel family: calls, total ms, average us and share, from rocprofv3's kernel statistics."""
    fam = {"k_demc_propose": "k_demc_propose", "k_demc_decide": "k_demc_decide", "tci_cohort_kernel": "likelihood",
           "tci_tile_kernel": "likelihood", "copyBuffer": "copies", "k_ce_": "group_reductions", "k_cr_": "group_reductions"}
    out = {}
    for r in csv.DictReader(open(path)):
        ns = float(r["TotalDurationNs"])
        name = next((v for k, v in fam.items() if k in r["Name"]), "other")
        e = out.setdefault(name, dict(calls=0, total_ms=0.0))
        e["calls"] += int(r["Calls"])
        e["total_ms"] += ns * 1e-6
    sampler = sum(out[k]["total_ms"] for k in ("k_demc_propose", "k_demc_decide", "likelihood") if k in out)
    for k, e in out.items():
        e["avg_us"] = 1e3 * e["total_ms"] / e["calls"]
        if k in ("k_demc_propose", "k_demc_decide", "likelihood"):
            e["share_of_sampler"] = e["total_ms"] / sampler
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--pop", type=int, default=64)
    ap.add_argument("--gens", type=int, default=2000)
    ap.add_argument("--thin", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(HERE, "demc_time.json"))
    a = ap.parse_args()
    if a.kernel_stats:
        out = json.load(open(a.out))
        out["kernel_split"] = dict(kernel_split(a.kernel_stats), note="one rocprofv3 --kernel-trace --stats run of "
                                   "--trace-only in a process of its own: the run above plus a warm-up of 27 launches")
        out["comparison"] = comparison()
        json.dump(out, open(a.out, "w"), indent=1)
        print(json.dumps(out["kernel_split"]))
        return
    from transcriptioncycleinference_amd import Likelihood, mcmc, testdata

    cl = testdata()
    burn = a.gens // 2
    with Likelihood(cl, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
        mcmc.demc(lk, n_pop=a.pop, n_gen=4, thin=1, cells=[0, 1])   # warm-up
        t0 = time.perf_counter()
        res, sp = mcmc.demc(lk, n_pop=a.pop, n_gen=a.gens, thin=a.thin, n_burn=burn, seed=0)
        wall = time.perf_counter() - t0
        if a.trace_only:
            print(json.dumps(dict(device_ms=res.kernel_ms, wall_s=wall)))
            return
        K, ld = len(sp.cells), res.pop.shape[2]
        pop = res.pop.reshape(K * a.pop, ld)
        cid = np.repeat(np.array(sp.cells, np.int32), a.pop)
        half = [np.concatenate([np.arange(k * a.pop + h, (k + 1) * a.pop, 2) for k in range(K)]) for h in (0, 1)]
        fl = floor_ms(lk, pop, cid, 1) + sum(floor_ms(lk, pop[ix], cid[ix], a.gens) for ix in half)
    sel = a.thin * np.arange(res.chain.shape[0]) >= burn
    ss = res.sschain[sel].reshape(sel.sum(), K, a.pop)
    P = 7 + cl.lengths[np.array(sp.cells)]
    rmax = np.array([np.nanmax(np.append(res.rhat.rhat[k, :P[k]], res.rhat.s2_rhat[k])) for k in range(K)])
    emin = np.array([np.nanmin(np.append(res.ess.ess[k, :P[k]], res.ess.s2_ess[k])) for k in range(K)])
    q = lambda x: [float(v) for v in np.percentile(x, [5, 50, 95])]  # noqa: E731
    out = dict(dataset=cl.name, n_cells=K, n_pop=a.pop, n_gen=a.gens, thin=a.thin, n_burn=burn,
               device_ms=res.kernel_ms, wall_s=wall, floor_ms=fl, ratio_to_floor=res.kernel_ms / fl,
               launches=3 + 6 * a.gens, n_evals=int(res.n_evals.sum()),
               rhat_max_p5_p50_p95=q(rmax), cells_rhat_above_1p1=int((rmax > 1.1).sum()), ess_min_p5_p50_p95=q(emin),
               mean_ss_p5_p50_p95=q(ss.mean(axis=(0, 2))), accept_rate_p5_p50_p95=q(res.accept_rate.mean(axis=1)),
               oob_share=float(res.n_oob.sum() / (K * a.pop * a.gens)),
               comparison=comparison(),
               note="one run each, HIP events; the floor is bare likelihood launches on the final population")
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
