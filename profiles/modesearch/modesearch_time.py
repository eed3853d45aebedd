"""Time the mode search on TestData next to its floor, and measure what starting the chains from it does.

Workload: the 299 TestData cells, populations of --pops (64 and 256) members, --gens (500) generations. Records
  * the device time of the search (its HIP events) and the wall time of the call,
  * the floor: n_gen + 1 bare launches of the batched likelihood kernel on the same row count, timed with events in the
    same process, and the ratio of the search to it (the launches run on the initial population; the same count on the
    final population is recorded beside it, since the kernel's time depends on theta),
  * per cell f0_best (the best start), f_best and ss_best of the search, and the best SS and lp any of the replicates of
    a plain fit reached (MCMClp's ss_min and lp_best),
  * the fit comparison: --replicates (4) replicates, --steps (20,000) steps, half of them burn-in, every --thin-th
    (10th) row kept, seed 0 -- the run of profiles/temper -- with presearch (the first of --pops) and without: per cell
    the largest R-hat, ss_gap and the best replicate's mean SS.
Writes profiles/modesearch/modesearch_time.json (or --out) with the commit it ran on.

    python profiles/modesearch/modesearch_time.py [--steps 20000] [--replicates 4] [--pops 64 256] [--gens 500]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch  # the HIP runtime before libtci.so, as bench.py loads it

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from transcriptioncycleinference_amd import Likelihood, mcmc, testdata  # noqa: E402


def commit():
    """HEAD, with "+changes" when the tree differs from it; --commit names it where the tree has no history."""
    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "-uno"], capture_output=True, text=True,
                               check=True).stdout.strip()
        return head + ("+changes" if dirty else "")
    except Exception:
        return "unknown"


def quart(x):
    x = np.asarray(x, np.float64)
    x = x[np.isfinite(x)]
    return [float(v) for v in np.percentile(x, [25, 50, 75])] if x.size else None


def floor_ms(lk, pop0, cid, launches):
    """Device ms of `launches` bare likelihood launches on the rows of pop0 [K, n_pop, ld]."""
    K, n_pop, ld = pop0.shape
    th = torch.from_numpy(pop0.reshape(K * n_pop, ld)).cuda()
    ids = torch.from_numpy(np.repeat(cid, n_pop).astype(np.int32)).cuda()
    out = torch.empty(K * n_pop, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream()
    for _ in range(5):
        lk.ss_batch_device(th, ids, out, stream=st)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(launches):
        lk.ss_batch_device(th, ids, out, stream=st)
    e1.record(st)
    e1.synchronize()
    return float(e0.elapsed_time(e1))


def timed_fit(lk, a, **kw):
    t0 = time.perf_counter()
    fr = mcmc.fit(lk, n_steps=a.steps, n_burn=a.steps // 2, thin=a.thin, seed=a.seed, cells=range(a.cells),
                  replicates=a.replicates, logpost=True, **kw)
    return fr, dict(wall_s=time.perf_counter() - t0, device_ms=float(fr.elapsed_ms), n_evals=int(fr.n_evals))


def convergence(fr):
    rh = [e["rhat_max"] for e in fr.MCMCrhat]
    gap = [e["ss_gap"] for e in fr.MCMClp]
    best = [float(np.min(e["ss_mean"])) for e in fr.MCMClp]
    return dict(rhat_max=quart(rh), rhat_max_above_1p1=int(sum(r > 1.1 for r in rh)), ss_gap=quart(gap),
                best_replicate_ss_mean=quart(best), per_cell=dict(rhat_max=rh, ss_gap=gap, best_replicate_ss_mean=best))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--replicates", type=int, default=4)
    ap.add_argument("--thin", type=int, default=10)
    ap.add_argument("--cells", type=int, default=299)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--pops", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--gens", type=int, default=500)
    ap.add_argument("--no-fits", action="store_true", help="time the search alone (e.g. under a kernel trace)")
    ap.add_argument("--out", default=os.path.join(HERE, "modesearch_time.json"))
    ap.add_argument("--commit", default=None, help="the commit to record (default: asked of git)")
    a = ap.parse_args()
    out = dict(commit=a.commit or commit(), args={k: v for k, v in vars(a).items() if k not in ("commit", "out", "no_fits")})
    with Likelihood(testdata(), "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
        mcmc.modesearch(lk, n_pop=8, n_gen=5, seed=a.seed, cells=range(a.cells))   # warm-up
        out["search"] = {}
        first = None
        for n_pop in a.pops:
            t0 = time.perf_counter()
            sr, sp = mcmc.modesearch(lk, n_pop=n_pop, n_gen=a.gens, seed=a.seed, cells=range(a.cells))
            wall = time.perf_counter() - t0
            fl = floor_ms(lk, sp.pop0, np.array(sp.cells, np.int32), a.gens + 1)
            fl_end = floor_ms(lk, sr.pop, np.array(sp.cells, np.int32), a.gens + 1)   # the SS cost depends on theta
            acc = sr.n_accepted.sum(axis=1) / float(sr.n_accepted.shape[1] * n_pop)
            out["search"][str(n_pop)] = dict(
                device_ms=sr.kernel_ms, wall_s=wall, n_evals=sr.n_evals, floor_ms=fl, ratio_to_floor=sr.kernel_ms / fl,
                floor_final_population_ms=fl_end,
                f0_best=quart(sr.f_trace[0]), f_best=quart(sr.f_best), ss_best=quart(sr.ss_best),
                accept_rate_first_last_10=[float(acc[:10].mean()), float(acc[-10:].mean())],
                per_cell=dict(f0_best=sr.f_trace[0].tolist(), f_best=sr.f_best.tolist(), ss_best=sr.ss_best.tolist()))
            first = first or n_pop
        if a.no_fits:
            print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk != "per_cell"} for k, v in out["search"].items()}))
            return
        fr_p, out["plain_fit"] = timed_fit(lk, a)
        fr_s, out["presearch_fit"] = timed_fit(lk, a, presearch=dict(n_pop=first, n_gen=a.gens))
    out["presearch_fit"]["n_pop"] = first
    out["plain_fit"].update(convergence(fr_p))
    out["presearch_fit"].update(convergence(fr_s))
    out["plain_fit"]["per_cell"].update(ss_min=[float(np.min(e["ss_min"])) for e in fr_p.MCMClp],
                                        lp_best=[float(np.max(e["lp_best"])) for e in fr_p.MCMClp])
    out["plain_fit"]["ss_min"] = quart(out["plain_fit"]["per_cell"]["ss_min"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: ({kk: vv for kk, vv in v.items() if kk != "per_cell"} if isinstance(v, dict) else v)
                      for k, v in out.items() if k != "search"}))
    print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk != "per_cell"} for k, v in out["search"].items()}))


if __name__ == "__main__":
    main()
