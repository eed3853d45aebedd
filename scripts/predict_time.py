"""Wall time of Likelihood.predict (bands reduced on the device) against the host route it replaces:
Likelihood.forward on every sample row, then the plims rule in numpy.

python scripts/predict_time.py [--reps 5] [--out profiles/predict/predict_time.json]

Case 1: TestData, 299 cells x S = 500 samples, probs (0.025, 0.5, 0.975), raw grid, both routes in one
process, alternating. Case 2: predict alone at 10,000 synthetic 200-point cells x 500 samples; the
host route there would hold 2 x 10,000 x 500 x 200 doubles = 16 GB of simulated rows and is skipped
unless that fits in free memory. Times are host clocks around synchronous calls (each ends in a
stream synchronise); median and min-max over the repeats after one warm-up of each route.
The device time of k_quantile alone is not reported: the ABI has no event hook for it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (its HIP runtime loads before libtci.so, as in bench.py)

from transcriptioncycleinference_amd import Likelihood, from_lists, testdata  # noqa: E402
from transcriptioncycleinference_amd.data import draw_x0, synthetic_cells  # noqa: E402

PROBS = (0.025, 0.5, 0.975)


def host_route(lk, theta, cid, probs):
    n_sel, S, ld = theta.shape
    ms2, pp7 = lk.forward(theta.reshape(n_sel * S, ld), np.repeat(cid, S), grid="raw")
    out = []
    for sim in (ms2, pp7):
        x = np.sort(sim.reshape(n_sel, S, -1), axis=1)
        bands = np.empty((n_sel, len(probs), x.shape[2]))
        with np.errstate(invalid="ignore"):
            for q, p in enumerate(probs):
                h = (S - 1) * p
                lo = int(np.floor(h))
                f = h - lo
                bands[:, q] = x[:, lo] + f * (x[:, lo + 1] - x[:, lo]) if lo + 1 < S else x[:, S - 1]
        for k, c in enumerate(cid):   # NaN past a cell's N, as predict writes it
            bands[k, :, int(lk.lengths[c]):] = np.nan
        out.append(bands)
    return out


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t0)
    return r, {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)), "reps": reps}


def sample_theta(rng, lengths, cid, S):
    ld = 7 + int(lengths[cid].max())
    theta = np.zeros((len(cid), S, ld))
    for k, c in enumerate(cid):
        base = draw_x0(rng, int(lengths[c]))
        theta[k, :, :len(base)] = base + rng.normal(0, 0.05, (S, len(base))) * np.abs(base)
    return theta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--synthetic-cells", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict", "predict_time.json"))
    a = ap.parse_args()
    S = 500
    res = {"probs": PROBS, "S": S, "timer": "host perf_counter around synchronous calls", "k_quantile_device_ms": None}
    rng = np.random.default_rng(20201028)

    cl = testdata()
    cid = np.arange(cl.n_cells, dtype=np.int32)
    theta = sample_theta(rng, cl.lengths, cid, S)
    with Likelihood(cl, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
        got = lk.predict(theta, cid, probs=PROBS)       # warm-up of both routes
        want = host_route(lk, theta, cid, PROBS)
        same = all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want))
        tp, th = [], []
        for _ in range(a.reps):                          # alternating
            tp.append(timed(lambda: lk.predict(theta, cid, probs=PROBS), 1)[1]["median_s"])
            th.append(timed(lambda: host_route(lk, theta, cid, PROBS), 1)[1]["median_s"])
        stat = lambda t: {"median_s": float(np.median(t)), "min_s": float(min(t)), "max_s": float(max(t)),  # noqa: E731
                          "reps": len(t)}
        res["testdata"] = {"cells": int(cl.n_cells), "rows": int(cl.n_cells) * S, "predict": stat(tp),
                           "forward_plus_numpy": stat(th), "results_equal": bool(same),
                           "speedup_median": float(np.median(th) / np.median(tp))}
    print(json.dumps(res["testdata"]), flush=True)

    nc, npts = a.synthetic_cells, 200

    def fwd(times, th):
        nan = [np.full(len(t), np.nan) for t in times]
        with Likelihood(from_lists([(t, x, x) for t, x in zip(times, nan)]), "P2P-MS2v5-LacZ-PP7v4", device=0) as L:
            return L.forward(th, np.arange(len(times), dtype=np.int32), grid="interp")

    syn, _ = synthetic_cells(nc, npts, 20201028, fwd)
    cid = np.arange(nc, dtype=np.int32)
    theta = sample_theta(rng, syn.lengths, cid, S)
    host_bytes = 2 * nc * S * npts * 8
    with Likelihood(syn, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
        lk.predict(theta[:64], cid[:64], probs=PROBS)   # warm-up
        _, st = timed(lambda: lk.predict(theta, cid, probs=PROBS), max(2, a.reps // 2))
    res["synthetic"] = {"cells": nc, "points": npts, "rows": nc * S, "predict": st,
                        "theta_bytes_uploaded": int(theta.nbytes), "band_bytes_downloaded": 2 * nc * len(PROBS) * npts * 8,
                        "forward_plus_numpy": f"skipped: its {host_bytes / 1e9:.0f} GB of simulated rows on the host "
                                              "(plus the sorted copy) were not attempted"}
    print(json.dumps(res["synthetic"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
