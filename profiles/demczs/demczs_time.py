"""Time the DE-MC(zs) sampler on TestData and summarise what it samples; time its proposal kernel against DE-MC's.

    python profiles/demczs/demczs_time.py --full [--chains 8] [--gens 16000] [--thin 10] [--presearch-gens 100]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o full -- python profiles/demczs/demczs_time.py --full-trace
    python profiles/demczs/demczs_time.py --kernel-stats DIR/.../full_kernel_stats.csv   (merges the split into --out)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o zs -- python profiles/demczs/demczs_time.py --trace-only
    python profiles/demczs/demczs_time.py --kernel-trace DIR/.../zs_kernel_trace.csv   (merges "propose" into --out)

--full, one process: mcmc.demczs on all 299 cells, default options, seed 0, --chains chains for --gens generations, every
--thin-th kept, the first half burn-in (the evaluation count of DESIGN.md 7m's DE-MC run), once from search_population
and once from the final population of a mode search of m0 members and --presearch-gens generations. Per run: device
time (HIP events) and its ratio to the same number of bare likelihood launches on the same rows; the out-of-bounds, null
and accept fractions; per cell the largest classic R-hat, the largest rhat_rank, the least ESS and the mean SS of the
kept rows past burn-in, as [5th, 50th, 95th percentile] over the cells, beside profiles/demc/demc_time.json's own
figures and its DRAM comparison rows, copied as they stand. One run each; no spread is quoted. --full-trace runs the
search_population start alone for a kernel trace of its own, and --kernel-stats adds the three kernels' times from it.

The proposal kernel against DE-MC's:

--trace-only runs, on the first --cells cells of TestData and in one process, --repeats times: mcmc.demc with 2 * --rows
members (a half-sweep moves --rows rows per cell) and mcmc.demczs with --rows chains (every chain moves), --gens
generations each, default options, seed 0; a warm-up of two such repeats comes first. --kernel-trace reads that
run's dispatch records, drops the warm-up's, splits every kernel's dispatches into the repeats in time order and writes
per kernel and repeat the total time, the dispatches and the time per row, with the spread over the repeats. The time
condition of DESIGN.md 7p is k_zs_propose's time per row against k_demc_propose's. To separate what the difference is
made of, the same process then runs three variants of DE-MC(zs), --repeats times each: p_snooker = 0 (no snooker rows);
p_snooker = 0 on an archive of the 64 rows DE-MC's population starts from, never appended to (L2-resident as DE-MC's
population is, and the same differences); and that small archive with the default p_snooker. Then both samplers run
on a start where almost no proposal leaves the box, so that either proposal kernel sums the prior on nearly all its
rows: a Gaussian prior per coordinate (centre of the box, a 16th of its width, bounds at +-8 sigma), sigma2_0 = 1e12
without updatesigma (a flat likelihood), 64 rows per cell drawn from it: DE-MC on the 64 (demc_gauss), DE-MC(zs) with
32 chains on that 64-row archive, never appended to, with p_snooker = 0 (zs_gauss_p0_m64) and the default. With no
snooker row, an L2-resident archive and the prior on every row of both, what is left between zs_gauss_p0_m64 and
demc_gauss is what the two kernels' code does differently per row: the second index call q (one Philox-10 per lane), the
ljac and move stores. The dispatches follow the main ones in time order."""
import argparse
import csv
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

KERNELS = {"k_demc_propose<false>": "k_demc_propose", "k_zs_propose<false, false": "k_zs_propose",
           "k_demc_decide<false>": "k_demc_decide", "k_zs_decide<false, false": "k_zs_decide"}


FAM = {"k_zs_propose": "k_zs_propose", "k_zs_decide": "k_zs_decide", "tci_cohort_kernel": "likelihood",
       "tci_tile_kernel": "likelihood", "copyBuffer": "copies", "k_ce_": "group_reductions", "k_cr_": "group_reductions",
       "k_ck_": "group_reductions", "k_ms_": "mode_search"}
VARIANTS = ("zs_p0", "zs_p0_m64", "zs_m64", "zs_gauss_p0_m64", "zs_gauss_m64")   # demc_gauss runs between the last two groups


def floor_ms(lk, rows, cid, launches):
    import torch

    th = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    c = torch.from_numpy(np.ascontiguousarray(cid)).cuda()
    out = torch.empty(len(cid), dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream()
    lk.ss_batch_device(th, c, out, stream=st)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        lk.ss_batch_device(th, c, out, stream=st)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def full(a):
    import time

    import torch  # noqa: F401  the HIP runtime before libtci.so, as bench.py loads it

    from transcriptioncycleinference_amd import Likelihood, mcmc, testdata

    cl = testdata()
    burn = a.gens // 2
    q = lambda x: [float(v) for v in np.nanpercentile(x, [5, 50, 95])]  # noqa: E731
    runs = {}
    with Likelihood(cl, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
        mcmc.demczs(lk, n_pop=a.chains, n_gen=4, thin=1, cells=[0, 1])   # warm-up
        starts = [("search_population", None)] + ([] if a.full_trace else [("mode_search", dict(n_gen=a.presearch_gens))])
        for name, ps in starts:
            t0 = time.perf_counter()
            res, sp = mcmc.demczs(lk, n_pop=a.chains, n_gen=a.gens, thin=a.thin, n_burn=burn, seed=0, presearch=ps,
                                  rank=not a.full_trace)
            wall = time.perf_counter() - t0
            if a.full_trace:
                print(json.dumps(dict(device_ms=res.kernel_ms, wall_s=wall)))
                return
            K, ld = len(sp.cells), res.pop.shape[2]
            cid = np.repeat(np.array(sp.cells, np.int32), a.chains)
            fl = floor_ms(lk, res.pop.reshape(K * a.chains, ld), cid, 1 + a.gens)
            sel = a.thin * np.arange(res.chain.shape[0]) >= burn
            ss = res.sschain[sel].reshape(sel.sum(), K, a.chains)
            P = 7 + cl.lengths[np.array(sp.cells)]
            rmax = np.array([np.nanmax(np.append(res.rhat.rhat[k, :P[k]], res.rhat.s2_rhat[k])) for k in range(K)])
            rrank = np.array([np.nanmax(np.append(res.rank.rhat_rank[k, :P[k]], res.rank.s2_rhat_rank[k])) for k in range(K)])
            emin = np.array([np.nanmin(np.append(res.ess.ess[k, :P[k]], res.ess.s2_ess[k])) for k in range(K)])
            moves = K * a.chains * a.gens
            runs[name] = dict(device_ms=res.kernel_ms, wall_s=wall, floor_ms=fl, ratio_to_floor=res.kernel_ms / fl,
                              launches=3 + 3 * a.gens, n_evals=int(res.n_evals.sum()), m0=int(res.m0),
                              n_archive=int(res.n_archive), presearch_gens=ps["n_gen"] if ps else 0,
                              rhat_max_p5_p50_p95=q(rmax), cells_rhat_above_1p1=int((rmax > 1.1).sum()),
                              rhat_rank_max_p5_p50_p95=q(rrank), cells_rhat_rank_above_1p01=int((rrank > 1.01).sum()),
                              ess_min_p5_p50_p95=q(emin), mean_ss_p5_p50_p95=q(ss.mean(axis=(0, 2))),
                              accept_rate_p5_p50_p95=q(res.accept_rate.mean(axis=1)),
                              oob_share=float(res.n_oob.sum() / moves), null_share=float(res.n_null.sum() / moves))
            print(name, json.dumps(runs[name]), flush=True)
            del res
    dm = json.load(open(os.path.join(HERE, "..", "demc", "demc_time.json")))
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out["full"] = dict(dataset=cl.name, n_cells=cl.n_cells, chains=a.chains, n_gen=a.gens, thin=a.thin, n_burn=burn, runs=runs,
                       demc={k: v for k, v in dm.items() if k not in ("comparison", "kernel_split")},
                       demc_kernel_split=dm.get("kernel_split"), comparison=dm.get("comparison"),
                       note="one run each, HIP events; the floor is 1 + n_gen bare likelihood launches on the final states; "
                            "demc and comparison are profiles/demc/demc_time.json's, copied as they stand")
    json.dump(out, open(a.out, "w"), indent=1)


def kernel_stats(a):
    split = {}
    for r in csv.DictReader(open(a.kernel_stats)):
        name = next((v for k, v in FAM.items() if k in r["Name"]), "other")
        e = split.setdefault(name, dict(calls=0, total_ms=0.0))
        e["calls"] += int(r["Calls"])
        e["total_ms"] += float(r["TotalDurationNs"]) * 1e-6
    three = ("k_zs_propose", "k_zs_decide", "likelihood")
    tot = sum(split[k]["total_ms"] for k in three if k in split)
    for k, e in split.items():
        e["avg_us"] = 1e3 * e["total_ms"] / e["calls"]
        if k in three:
            e["share_of_sampler"] = e["total_ms"] / tot
    out = json.load(open(a.out))
    out["full"]["kernel_split"] = dict(split, note="one rocprofv3 --kernel-trace --stats run of --full-trace in a process of "
                                       "its own: the search_population start plus the warm-up's launches")
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out["full"]["kernel_split"]))


def trace(a):
    import torch  # noqa: F401  the HIP runtime before libtci.so, as bench.py loads it

    from transcriptioncycleinference_amd import Likelihood, mcmc, testdata

    cl = testdata()
    ids = list(range(a.cells))
    with Likelihood(cl, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
        m0 = mcmc.demczs_m0(cl, ids)
        sp = mcmc.search_population(cl, ids, 0, m0)
        run_zs = lambda g: lk.demczs(sp.pop0[:, :a.rows], sp.pop0, np.array(sp.cells, np.int32), sp.lower, sp.upper,  # noqa: E731
                                     sp.prior_mu, sp.prior_sig, mcmc.demc_jitter(cl, sp.cells), n_gen=g, thin=0, seed=0)
        run_dm = lambda g: mcmc.demc(lk, n_pop=2 * a.rows, n_gen=g, thin=0, seed=0, cells=ids, rhat=False, ess=False)[0]  # noqa: E731
        for _ in range(2):   # a warm-up as long as two repeats: the first launches of a process run at lower clocks
            run_dm(a.gens), run_zs(a.gens)
        out = dict(cells=a.cells, rows_per_cell=a.rows, gens=a.gens, repeats=a.repeats, m0=m0, demc_ms=[], demczs_ms=[],
                   zs_oob=[], zs_null=[], zs_accept=[], demc_oob=[])
        for _ in range(a.repeats):
            d, z = run_dm(a.gens), run_zs(a.gens)
            out["demc_ms"].append(d.kernel_ms)
            out["demczs_ms"].append(z.kernel_ms)
            out["demc_oob"].append(float(d.n_oob.sum() / (d.n_oob.size * a.gens)))
            out["zs_oob"].append(float(z.n_oob.sum() / (z.n_oob.size * a.gens)))
            out["zs_null"].append(float(z.n_null.sum() / (z.n_null.size * a.gens)))
            out["zs_accept"].append(float(z.accept_rate.mean()))
        small = mcmc.search_population(cl, ids, 0, 2 * a.rows)    # the 64 rows DE-MC's population starts from
        never = 10 ** 9
        run_v = dict(
            zs_p0=lambda: lk.demczs(sp.pop0[:, :a.rows], sp.pop0, np.array(sp.cells, np.int32), sp.lower, sp.upper, sp.prior_mu,
                                    sp.prior_sig, mcmc.demc_jitter(cl, sp.cells), n_gen=a.gens, thin=0, seed=0, p_snooker=0.0),
            zs_p0_m64=lambda: lk.demczs(small.pop0[:, :a.rows], small.pop0, np.array(sp.cells, np.int32), sp.lower, sp.upper,
                                        sp.prior_mu, sp.prior_sig, mcmc.demc_jitter(cl, sp.cells), n_gen=a.gens, thin=0,
                                        seed=0, p_snooker=0.0, append_every=never),
            zs_m64=lambda: lk.demczs(small.pop0[:, :a.rows], small.pop0, np.array(sp.cells, np.int32), sp.lower, sp.upper,
                                     sp.prior_mu, sp.prior_sig, mcmc.demc_jitter(cl, sp.cells), n_gen=a.gens, thin=0, seed=0,
                                     append_every=never))
        # the Gaussian start: nothing leaves the box, so both proposal kernels sum the prior on (nearly) every row
        K, ld = len(sp.cells), sp.pop0.shape[2]
        cid = np.array(sp.cells, np.int32)
        glo, gup = np.full((K, ld), -np.inf), np.full((K, ld), np.inf)
        gmu, gsig, gpop = np.zeros((K, ld)), np.full((K, ld), np.inf), np.zeros((K, 2 * a.rows, ld))
        for k, c in enumerate(sp.cells):
            P = 7 + int(cl.lengths[c])
            lo = np.concatenate([[0, 0, 0, 0, 0, 0, 0], np.full(P - 7, -30.0)])
            up = np.concatenate([[10, 20, 10, 50, 50, 1, 40], np.full(P - 7, 30.0)])
            gmu[k, :P], gsig[k, :P] = (lo + up) / 2, (up - lo) / 16
            glo[k, :P], gup[k, :P] = gmu[k, :P] - 8 * gsig[k, :P], gmu[k, :P] + 8 * gsig[k, :P]
            gpop[k, :, :P] = gmu[k, :P] + gsig[k, :P] * np.random.default_rng([5, c]).standard_normal((2 * a.rows, P))
        gjit = np.where(np.isfinite(gsig), 0.01 * gsig, 0.0)
        gkw = dict(sigma2_0=1e12, updatesigma=False, n_gen=a.gens, thin=0, seed=0)
        run_v["zs_gauss_p0_m64"] = lambda: lk.demczs(gpop[:, :a.rows], gpop, cid, glo, gup, gmu, gsig, gjit, p_snooker=0.0,
                                                     append_every=never, **gkw)
        run_v["zs_gauss_m64"] = lambda: lk.demczs(gpop[:, :a.rows], gpop, cid, glo, gup, gmu, gsig, gjit,
                                                  append_every=never, **gkw)
        out["variants"] = {}
        for v in VARIANTS:
            if v == "zs_gauss_m64":     # DE-MC on the same start, between the two DE-MC(zs) groups
                for _ in range(a.repeats):
                    d = lk.demc(gpop, cid, glo, gup, gmu, gsig, gjit, **gkw)
                out["variants"]["demc_gauss"] = dict(oob=float(d.n_oob.sum() / (d.n_oob.size * a.gens)),
                                                     accept=float(d.accept_rate.mean()), device_ms=d.kernel_ms)
            for _ in range(a.repeats):
                z = run_v[v]()
            out["variants"][v] = dict(oob=float(z.n_oob.sum() / (z.n_oob.size * a.gens)),
                                      null=float(z.n_null.sum() / (z.n_null.size * a.gens)),
                                      accept=float(z.accept_rate.mean()), device_ms=z.kernel_ms)
    print(json.dumps(out))


def reduce(a):
    disp = {v: [] for v in KERNELS.values()}
    for r in csv.DictReader(open(a.kernel_trace)):
        name = next((v for k, v in KERNELS.items() if k in r["Kernel_Name"]), None)
        if name:
            disp[name].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows = a.cells * a.rows
    per = dict(k_demc_propose=2 * a.gens, k_demc_decide=2 * a.gens, k_zs_propose=a.gens, k_zs_decide=a.gens)
    warm = {k: 2 * v for k, v in per.items()}   # the warm-up: two repeats of either
    out = dict(cells=a.cells, rows_per_launch=rows, gens=a.gens, repeats=a.repeats, kernels={})
    variants = {}
    for k, d in disp.items():
        d = sorted(d)[warm[k]:]
        if k.startswith("k_zs"):     # the variants' dispatches follow the main runs'
            assert len(d) == per[k] * a.repeats * (1 + len(VARIANTS)), (k, len(d))
            for vi, v in enumerate(VARIANTS):
                dv = d[per[k] * a.repeats * (1 + vi):per[k] * a.repeats * (2 + vi)]
                ns = [1e3 * sum(e - s for s, e in dv[i * per[k]:(i + 1) * per[k]]) * 1e-3 / (per[k] * rows)
                      for i in range(a.repeats)]
                variants.setdefault(v, {})[k] = dict(ns_per_row=ns, ns_per_row_mean=float(np.mean(ns)),
                                                     ns_per_row_spread=float(max(ns) - min(ns)))
            d = d[:per[k] * a.repeats]
        else:                        # DE-MC's second group: the Gaussian start
            assert len(d) == per[k] * a.repeats * 2, (k, len(d))
            dv = d[per[k] * a.repeats:]
            ns = [sum(e - s for s, e in dv[i * per[k]:(i + 1) * per[k]]) / (per[k] * rows) for i in range(a.repeats)]
            variants.setdefault("demc_gauss", {})[k] = dict(ns_per_row=ns, ns_per_row_mean=float(np.mean(ns)),
                                                            ns_per_row_spread=float(max(ns) - min(ns)))
            d = d[:per[k] * a.repeats]
        assert len(d) == per[k] * a.repeats, (k, len(d))
        us = [sum(e - s for s, e in d[i * per[k]:(i + 1) * per[k]]) * 1e-3 for i in range(a.repeats)]
        ns_row = [1e3 * u / (per[k] * rows) for u in us]
        out["kernels"][k] = dict(dispatches_per_repeat=per[k], total_us=us, ns_per_row=ns_row,
                                 ns_per_row_mean=float(np.mean(ns_row)), ns_per_row_spread=float(max(ns_row) - min(ns_row)))
    zs, dm = out["kernels"]["k_zs_propose"], out["kernels"]["k_demc_propose"]
    out["propose_ratio_zs_to_demc"] = zs["ns_per_row_mean"] / dm["ns_per_row_mean"]
    out["no_worse_within_spread"] = bool(zs["ns_per_row_mean"] <= dm["ns_per_row_mean"] + zs["ns_per_row_spread"]
                                         + dm["ns_per_row_spread"])
    out["variants"] = variants
    if a.run_json:
        out["run"] = json.load(open(a.run_json))
    whole = json.load(open(a.out)) if os.path.exists(a.out) else {}
    whole = {k: v for k, v in whole.items() if k in ("full", "propose")}   # an earlier layout held the trace at top level
    whole["propose"] = out
    json.dump(whole, open(a.out, "w"), indent=1)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--full-trace", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--thin", type=int, default=10)
    ap.add_argument("--presearch-gens", type=int, default=100)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--run-json", default=None, help="the line --trace-only printed, saved to a file")
    ap.add_argument("--cells", type=int, default=64)
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--gens", type=int, default=None, help="default 300, with --full / --full-trace 16000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "demczs_time.json"))
    a = ap.parse_args()
    if a.gens is None:
        a.gens = 16000 if a.full or a.full_trace else 300
    if a.full or a.full_trace:
        full(a)
    elif a.kernel_stats:
        kernel_stats(a)
    elif a.kernel_trace:
        reduce(a)
    else:
        trace(a)


if __name__ == "__main__":
    main()
