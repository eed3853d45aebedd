#!/usr/bin/env python3
"""A/B in one process: the bench launch (299 TestData cells x 256 proposals, 8 resident proposal
batches cycled) on the shipped library and on another build of it (default build/ab/libtci_old.so:
the previous commit's tci_kernels.hip, `python scripts/ab_variants.py --build --variants ...` or a
copy), alternated round by round. Both contexts hold the same cells; the SS of every batch must be
equal bit for bit. Reports per build the median, quartiles and range of the per-launch µs (HIP events
around `launches` back-to-back launches per round) and every round's value, the paired differences
(other - shipped, same round), and the same for two probes of the bench batch: every row rejected
(wave launch + flag read only) and the in-bounds rows alone, compacted.
usage: python scripts/lk_prologue_ab.py [--other LIB] [--rounds 15] [--launches 40] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from transcriptioncycleinference_amd import Likelihood, testdata  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--other", default=os.path.join(ROOT, "build", "ab", "libtci_old.so"))
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--launches", type=int, default=40)
ap.add_argument("--out", default=None)
a = ap.parse_args()

cells = testdata()
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream(dev)
lks = {"other": Likelihood(cells, bench.CONSTRUCT, 0, lib_path=a.other), "shipped": Likelihood(cells, bench.CONSTRUCT, 0)}
rounds = bench.ProposalRounds(cells, 256, 8, 20201028, dev)
outs = {}
for name, lk in lks.items():
    res = []
    for r in range(len(rounds.theta)):
        lk.ss_batch_device(rounds.theta[r], rounds.cid, rounds.out, rounds.active[r], stream=st)
        torch.cuda.synchronize()
        res.append(rounds.out.cpu().numpy().copy())
    outs[name] = np.stack(res)
equal = bool(np.array_equal(outs["other"].view(np.uint64), outs["shipped"].view(np.uint64)))


def timed(lk, theta, cid, out, active):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(a.launches):
        lk.ss_batch_device(theta, cid, out, active, stream=st)
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.launches * 1e3


def summary(ts):
    q1, med, q3 = (float(x) for x in np.percentile(ts, [25, 50, 75]))
    return {"median_us": med, "q1_us": q1, "q3_us": q3, "min_us": float(np.min(ts)), "max_us": float(np.max(ts)),
            "rounds_us": [round(float(t), 3) for t in ts]}


def paired(t):
    d = np.array(t["other"]) - np.array(t["shipped"])
    return {"median_us": float(np.median(d)), "min_us": float(d.min()), "max_us": float(d.max()),
            "rounds_shipped_faster": int((d > 0).sum())}


act0 = rounds.active[0].cpu().numpy().astype(bool)
keep = torch.from_numpy(np.flatnonzero(act0)).to(dev)
probes = {"all_rejected": (rounds.theta[0], rounds.cid, rounds.out, torch.zeros_like(rounds.active[0])),
          "in_bounds_only": (rounds.theta[0][keep].contiguous(), rounds.cid[keep].contiguous(),
                             torch.empty(len(keep), dtype=torch.float64, device=dev),
                             torch.ones(len(keep), dtype=torch.uint8, device=dev))}
times = {"bench": {k: [] for k in lks}, **{p: {k: [] for k in lks} for p in probes}}
for lk in lks.values():  # warm-up
    bench.kernel_mode(lk, rounds, 64, st)
    for args in probes.values():
        timed(lk, *args)
for _ in range(a.rounds):
    for name, lk in lks.items():
        _, ms, _ = bench.kernel_mode(lk, rounds, a.launches, st)
        times["bench"][name].append(ms * 1e3)
for p, args in probes.items():
    for _ in range(a.rounds):
        for name, lk in lks.items():
            times[p][name].append(timed(lk, *args))
n_act = float(np.mean(rounds.n_active))
out = {"workload": f"TestData 299 cells x 256 proposals ({rounds.B} rows, {n_act:.0f} in bounds per launch)",
       "other": os.path.relpath(a.other, ROOT), "bitwise_equal": equal, "rounds": a.rounds,
       "launches_per_round": a.launches}
for case, t in times.items():
    out[case] = {k: summary(v) for k, v in t.items()}
    out[case]["other_minus_shipped"] = paired(t)
text = json.dumps(out, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
sys.exit(0 if equal else 1)
