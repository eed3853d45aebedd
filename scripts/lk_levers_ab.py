#!/usr/bin/env python3
"""A/B of several builds in one process, the method of scripts/lk_prologue_ab.py for more than two
libraries: the bench launch (299 TestData cells x 256 proposals, 8 resident proposal batches cycled)
on a parent build and on every other build given, alternated round by round. All contexts hold the
same cells; the SS of every batch must equal the parent's bit for bit. Reports per build the median,
quartiles and every round's per-launch µs (HIP events around `launches` back-to-back launches), the
paired differences against the parent (parent - build, same round; positive: the build is faster),
the parent's interquartile width -- the bar a paired median gain has to clear -- and the same for two
probes of the bench batch: every row rejected, and the in-bounds rows alone, compacted.
usage: python scripts/lk_levers_ab.py --libs parent=build/ab/libtci_old.so,A=...,shipped= [--rounds 25]
       [--launches 40] [--out FILE]      (an empty path: the in-tree libtci.so)"""
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
ap.add_argument("--libs", required=True, help="name=path,... ; the first one is the parent")
ap.add_argument("--rounds", type=int, default=25)
ap.add_argument("--launches", type=int, default=40)
ap.add_argument("--out", default=None)
a = ap.parse_args()

libs = [s.split("=", 1) for s in a.libs.split(",")]
parent = libs[0][0]
cells = testdata()
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream(dev)
lks = {n: Likelihood(cells, bench.CONSTRUCT, 0, lib_path=os.path.join(ROOT, p) if p else None) for n, p in libs}
rounds = bench.ProposalRounds(cells, 256, 8, 20201028, dev)
outs = {}
for name, lk in lks.items():
    res = []
    for r in range(len(rounds.theta)):
        rounds.out.fill_(-1.0)  # nothing may be left from another build's launch
        lk.ss_batch_device(rounds.theta[r], rounds.cid, rounds.out, rounds.active[r], stream=st)
        torch.cuda.synchronize()
        res.append(rounds.out.cpu().numpy().copy())
    outs[name] = np.stack(res)
equal = {n: bool(np.array_equal(outs[n].view(np.uint64), outs[parent].view(np.uint64))) for n in lks}


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
    return {"median_us": med, "q1_us": q1, "q3_us": q3, "iqr_us": q3 - q1, "min_us": float(np.min(ts)),
            "max_us": float(np.max(ts)), "rounds_us": [round(float(t), 3) for t in ts]}


def paired(t, n):
    d = np.array(t[parent]) - np.array(t[n])
    return {"median_gain_us": float(np.median(d)), "min_us": float(d.min()), "max_us": float(d.max()),
            "rounds_faster_than_parent": int((d > 0).sum())}


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
       "libs": dict(libs), "parent": parent, "bitwise_equal_to_parent": equal, "rounds": a.rounds,
       "launches_per_round": a.launches}
for case, t in times.items():
    out[case] = {k: summary(v) for k, v in t.items()}
    out[case]["parent_iqr_us"] = out[case][parent]["iqr_us"]
    out[case]["gain_over_parent"] = {n: paired(t, n) for n in lks if n != parent}
text = json.dumps(out, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
sys.exit(0 if all(equal.values()) else 1)
