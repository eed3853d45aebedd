"""Time k_zs_propose and k_zs_decide per row with the bounds census and the oriented reflection off and on.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o zs -- python profiles/bounds/bounds_time.py --trace-only [--parent]
    python profiles/bounds/bounds_time.py --kernel-trace DIR/.../zs_kernel_trace.csv --label this_a|parent_a|this_b|..

DESIGN.md 7p's kernel-trace procedure: the first 64 cells of TestData, 32 chains, m0 = 10 P of the longest of them,
300 generations, default options, seed 0, no kept rows; in one process two warm-up repeats and then three repeats of
every variant, one variant after the other:
  reject          Likelihood.demczs with its defaults: tci_demczs_run, the kernels without kBounds
  census          bounds='reject', census=True
  reflect         bounds='reflect'
  reflect_census  bounds='reflect', census=True
--parent runs the first variant alone (a tree without the new entry point; --tree names its root). --kernel-trace splits
every kernel's dispatches into the variants and repeats in time order and writes ns per row with the spread over the
repeats under --label into bounds_time.json. A label begins with `this` or `parent`; the processes of the two trees are
run alternately on one machine, the parent's first (parent_a, this_a, parent_b, this_b), because the first traced process
on a machine has been seen to run disturbed. With both trees present it adds the comparison of the `reject` variant:
the mean over each tree's processes, their difference, and whether it is within the spreads 7p reports for the two
kernels (0.048 and 0.075 ns per row); and the cost of the other variants over `reject`. The profiler run holds the
kernel trace alone."""
import argparse
import csv
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
VARIANTS = ("reject", "census", "reflect", "reflect_census")
KW = dict(reject={}, census=dict(census=True), reflect=dict(bounds="reflect"),
          reflect_census=dict(bounds="reflect", census=True))
SPREAD_7P = dict(k_zs_propose=0.048, k_zs_decide=0.075)   # ns per row, profiles/demczs/demczs_time.json


def trace(a):
    sys.path.insert(0, a.tree or os.path.join(HERE, "..", ".."))
    import torch  # noqa: F401  the HIP runtime before libtci.so, as bench.py loads it

    from transcriptioncycleinference_amd import Likelihood, mcmc, testdata

    cl = testdata()
    ids = list(range(a.cells))
    out = dict(cells=a.cells, rows_per_cell=a.rows, gens=a.gens, repeats=a.repeats, variants={})
    with Likelihood(cl, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
        m0 = mcmc.demczs_m0(cl, ids)
        sp = mcmc.search_population(cl, ids, 0, m0)
        jit = mcmc.demc_jitter(cl, sp.cells)
        run = lambda **kw: lk.demczs(sp.pop0[:, :a.rows], sp.pop0, np.array(sp.cells, np.int32), sp.lower, sp.upper,  # noqa: E731
                                     sp.prior_mu, sp.prior_sig, jit, n_gen=a.gens, thin=0, seed=0, **kw)
        for _ in range(2):   # a warm-up as long as two repeats: the first launches of a process run at lower clocks
            run()
        out["m0"] = m0
        for v in VARIANTS[:1] if a.parent else VARIANTS:
            ms = []
            for _ in range(a.repeats):
                z = run(**KW[v])
                ms.append(z.kernel_ms)
            out["variants"][v] = dict(device_ms=ms, oob=float(z.n_oob.sum() / (z.n_oob.size * a.gens)),
                                      accept=float(z.accept_rate.mean()))
    print(json.dumps(out))


def reduce(a):
    disp = dict(k_zs_propose=[], k_zs_decide=[])
    for r in csv.DictReader(open(a.kernel_trace)):
        for k in disp:
            if k + "<false" in r["Kernel_Name"]:     # every generation >= 1, with or without kBounds
                disp[k].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows = a.cells * a.rows
    variants = VARIANTS[:1] if a.label.startswith("parent") else VARIANTS
    out = dict(cells=a.cells, rows_per_launch=rows, gens=a.gens, repeats=a.repeats, kernels={})
    for k, d in disp.items():
        d = sorted(d)[2 * a.gens:]                   # the warm-up: two repeats
        assert len(d) == a.gens * a.repeats * len(variants), (k, len(d))
        for vi, v in enumerate(variants):
            dv = d[a.gens * a.repeats * vi:a.gens * a.repeats * (vi + 1)]
            ns = [sum(e - s for s, e in dv[i * a.gens:(i + 1) * a.gens]) / (a.gens * rows) for i in range(a.repeats)]
            out["kernels"].setdefault(v, {})[k] = dict(ns_per_row=ns, ns_per_row_mean=float(np.mean(ns)),
                                                       ns_per_row_spread=float(max(ns) - min(ns)))
    if a.run_json:
        out["run"] = json.load(open(a.run_json))
    whole = json.load(open(a.out)) if os.path.exists(a.out) else {}
    whole[a.label] = out
    ours, theirs = (sorted(w for w in whole if w.startswith(t)) for t in ("this", "parent"))
    if ours and theirs:
        cmp = {}
        for k, spread in SPREAD_7P.items():
            per = lambda ws, v: [whole[w]["kernels"][v][k]["ns_per_row_mean"] for w in ws]  # noqa: E731
            t, p = float(np.mean(per(ours, "reject"))), float(np.mean(per(theirs, "reject")))
            cmp[k] = dict(this_runs=per(ours, "reject"), parent_runs=per(theirs, "reject"), this=t, parent=p, difference=t - p,
                          spread_7p=spread, within_spread=bool(abs(t - p) <= spread))
            for v in VARIANTS[1:]:
                cmp[k][v + "_over_reject"] = float(np.mean(per(ours, v))) / t
        whole["comparison"] = cmp
    json.dump(whole, open(a.out, "w"), indent=1)
    print(json.dumps(whole.get("comparison", out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--parent", action="store_true")
    ap.add_argument("--tree", default=None, help="the root of the tree whose package runs (default: this one)")
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--label", default="this_a", help="this* or parent*: the tree and the process")
    ap.add_argument("--run-json", default=None, help="the line --trace-only printed, saved to a file")
    ap.add_argument("--cells", type=int, default=64)
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--gens", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "bounds_time.json"))
    a = ap.parse_args()
    if a.kernel_trace:
        reduce(a)
    else:
        trace(a)


if __name__ == "__main__":
    main()
