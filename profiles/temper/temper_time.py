"""Time a tempered fit of TestData next to the plain fit of the same chain count, and measure what the ladder does.

Workload: the 299 TestData cells, --replicates (4) replicates x --temper (4) rungs, --steps (20,000) steps, half of
them burn-in, every --thin-th (10th) row kept, against fit(replicates = replicates * temper) without tempering (the
same number of chains) and fit(replicates = replicates) (the plain run the cold rungs are compared with). Records
  * wall time and device time (the run's HIP events) of the three fits,
  * an upper estimate of the swap kernel's time per event: the device time of the tempered fit minus that of the same
    fit with swap_every = 0 (the ladder's rungs without swaps), over the number of events. The two fits walk
    different chains once states are exchanged, so the difference is confounded by their chain work (n_evals is
    recorded for both); k_swap has no timer of its own,
  * the per-pair swap rate: median and quartiles across cells, by pair,
  * the cold rungs' convergence beside the plain replicates': the cell's largest R-hat, ss_gap and smallest
    multi-chain ESS.
Writes profiles/temper/temper_time.json with the commit it ran on.

    python profiles/temper/temper_time.py [--steps 20000] [--replicates 4] [--temper 4] [--thin 10] [--cells 299]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch  # noqa: F401  (the HIP runtime before libtci.so, as bench.py loads it)

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
    if not x.size:
        return None
    return [float(v) for v in np.percentile(x, [25, 50, 75])]


def timed_fit(lk, a, **kw):
    t0 = time.perf_counter()
    fr = mcmc.fit(lk, n_steps=a.steps, n_burn=a.steps // 2, thin=a.thin, seed=a.seed, cells=range(a.cells), **kw)
    return fr, dict(wall_s=time.perf_counter() - t0, device_ms=float(fr.elapsed_ms), n_evals=int(fr.n_evals))


def convergence(fr):
    return dict(rhat_max=quart([e["rhat_max"] for e in fr.MCMCrhat]),
                rhat_max_above_1p1=int(sum(e["rhat_max"] > 1.1 for e in fr.MCMCrhat)),
                ess_min=quart([e["ess_min"] for e in fr.MCMCess]),
                ss_gap=quart([e["ss_gap"] for e in fr.MCMClp]),
                ss_mean=quart([np.min(e["ss_mean"]) for e in fr.MCMClp]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--replicates", type=int, default=4)
    ap.add_argument("--temper", type=int, default=4)
    ap.add_argument("--thin", type=int, default=10)
    ap.add_argument("--cells", type=int, default=299)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--commit", default=None, help="the commit to record (default: asked of git)")
    a = ap.parse_args()
    M, R = a.replicates, a.temper
    out = dict(commit=a.commit or commit(), args={k: v for k, v in vars(a).items() if k != "commit"})
    with Likelihood(testdata(), "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
        timed_fit(lk, argparse.Namespace(**{**vars(a), "steps": 200}), replicates=M, rhat=False)   # warm-up
        diag = dict(ess=True, logpost=True)
        fr_t, out["tempered"] = timed_fit(lk, a, replicates=M, temper=R, **diag)
        _, out["tempered_no_swaps"] = timed_fit(lk, a, replicates=M, temper=R, swap_every=0, rhat=False)
        _, out["plain_same_chain_count"] = timed_fit(lk, a, replicates=M * R, rhat=False)
        fr_p, out["plain"] = timed_fit(lk, a, replicates=M, **diag)
    ev = fr_t.MCMCtemper[0]["n_events"]
    out["swap_events"] = int(ev)
    out["swap_us_per_event"] = (1e3 * (out["tempered"]["device_ms"] - out["tempered_no_swaps"]["device_ms"]) / ev
                                if ev else None)
    rate = np.stack([e["swap_rate"] for e in fr_t.MCMCtemper])          # [cells, M, R - 1]
    out["swap_rate_by_pair"] = [quart(np.nanmean(rate[:, :, q], axis=1)) for q in range(R - 1)]
    out["beta_median_cell"] = [float(v) for v in np.median(np.stack([e["beta"] for e in fr_t.MCMCtemper]), axis=0)]
    out["accept_rate_by_rung"] = [quart(np.stack([e["accept_rate"] for e in fr_t.MCMCtemper])[:, :, q].mean(axis=1))
                                  for q in range(R)]
    out["cold_rungs"] = convergence(fr_t)
    out["plain_replicates"] = convergence(fr_p)
    with open(os.path.join(HERE, "temper_time.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
