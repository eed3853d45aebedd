"""Which coordinates reject DE-MC(zs)'s proposals at the box on TestData, and what oriented reflection does about it.

    timeout -k 10 600 python profiles/bounds/bounds_census.py --mode reject && \
    timeout -k 10 600 python profiles/bounds/bounds_census.py --mode reflect

DESIGN.md 7p's TestData run, exactly: all 299 cells, mcmc.demczs with default options, seed 0, 8 chains for 16,000
generations, every 10th kept, the first half burn-in, m0 = 1,360 (10 P of the longest cell), the drawn start
(search_population). Once in reject mode and once in reflect mode, the census on and every generation logged in both;
each mode is one process and writes its own entry of bounds_census.json.

Per mode, the rows of 7p's table: out of bounds / null / accepted shares, evaluations, per cell the largest classic R-hat,
the largest rhat_rank, the least ESS and the mean SS of the kept rows past burn-in as [5th, 50th, 95th percentile] over
the cells, and the device time (HIP events; one run, no spread).

The census, summed over cells and chains:
  leave_share         of all (proposal, coordinate) leaving events, the share of each of the seven scalars by name and of
                      the dR entries together, split below / above
  leave_per_crossing  oob / n_cross per scalar and for dR: the chance that a crossing coordinate leaves
  oob_share           reject mode: the share of the bounds-rejected proposals in which the coordinate had left (scalars by
                      name; dR_sum adds the dR entries' shares, so it exceeds 1 when several leave together)
  dR_by_position      the dR leaving events by the entry's relative position i / N in ten bins, below and above
  n_left_hist         the bounds-rejected proposals by their count of leaving coordinates (1, 2, 3, 4-7, 8+), and
                      exactly_one, the share with exactly one
  crossing_mean       crossing coordinates per non-null proposal
  near_wall           the share of kept dR values past burn-in within 1 of -30 and of +30 (is the posterior parked there?)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

NAMES = ("v", "tau", "ton", "MS2_basal", "PP7_basal", "A", "R")


def run(a):
    import torch  # noqa: F401  the HIP runtime before libtci.so, as bench.py loads it

    from transcriptioncycleinference_amd import Likelihood, mcmc, testdata

    cl = testdata()
    burn = a.gens // 2
    q = lambda x: [float(v) for v in np.nanpercentile(x, [5, 50, 95])]  # noqa: E731
    with Likelihood(cl, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
        mcmc.demczs(lk, n_pop=a.chains, n_gen=4, thin=1, cells=[0, 1], bounds=a.mode, census=True)   # warm-up
        t0 = time.perf_counter()
        res, sp = mcmc.demczs(lk, n_pop=a.chains, n_gen=a.gens, thin=a.thin, n_burn=burn, seed=0, rank=True, bounds=a.mode,
                              census=True, log_rows=a.gens)
        wall = time.perf_counter() - t0
    K, n_pop = len(sp.cells), a.chains
    N = cl.lengths[np.array(sp.cells)].astype(np.int64)
    P = 7 + N
    sel = a.thin * np.arange(res.chain.shape[0]) >= burn
    ss = res.sschain[sel].reshape(sel.sum(), K, n_pop)
    rmax = np.array([np.nanmax(np.append(res.rhat.rhat[k, :P[k]], res.rhat.s2_rhat[k])) for k in range(K)])
    rrank = np.array([np.nanmax(np.append(res.rank.rhat_rank[k, :P[k]], res.rank.s2_rhat_rank[k])) for k in range(K)])
    emin = np.array([np.nanmin(np.append(res.ess.ess[k, :P[k]], res.ess.s2_ess[k])) for k in range(K)])
    moves = K * n_pop * a.gens
    out = dict(mode=a.mode, device_ms=res.kernel_ms, wall_s=wall, n_evals=int(res.n_evals.sum()), m0=int(res.m0),
               oob_share_of_moves=float(res.n_oob.sum() / moves), null_share=float(res.n_null.sum() / moves),
               accept_share=float(res.accepted.sum() / moves), rhat_max_p5_p50_p95=q(rmax),
               cells_rhat_above_1p1=int((rmax > 1.1).sum()), rhat_rank_max_p5_p50_p95=q(rrank),
               cells_rhat_rank_above_1p01=int((rrank > 1.01).sum()), ess_min_p5_p50_p95=q(emin),
               mean_ss_p5_p50_p95=q(ss.mean(axis=(0, 2))), accept_rate_p5_p50_p95=q(res.accept_rate.mean(axis=1)))
    if a.mode == "reflect":
        out["reflected_share_of_moves"] = float(res.n_reflected.sum() / moves)
        out["reflections_per_reflected_proposal"] = float(res.n_refl.sum() / max((res.n_refl > 0).sum(), 1))
        out["orient_set_share"] = float(sum(res.orient[k, :, :P[k]].sum() for k in range(K)) / (n_pop * P.sum()))
    # the census: cells and chains summed
    nc, lo, hi = (np.where(x < 0, 0, x).astype(np.int64).sum(axis=1) for x in (res.n_cross, res.oob_lo, res.oob_hi))   # [K, ld]
    dr = np.arange(nc.shape[1])[None, :] >= 7
    real = np.arange(nc.shape[1])[None, :] < P[:, None]
    total = float((lo + hi).sum())
    rejected = float(res.n_oob.sum())
    cen = dict(leaving_events=int(total), crossings=int(nc.sum()), leave_share={}, leave_per_crossing={}, oob_share={})
    for j, name in enumerate(NAMES):
        cen["leave_share"][name] = dict(below=float(lo[:, j].sum() / total), above=float(hi[:, j].sum() / total))
        cen["leave_per_crossing"][name] = float((lo[:, j] + hi[:, j]).sum() / nc[:, j].sum())
        cen["oob_share"][name] = float((lo[:, j] + hi[:, j]).sum() / rejected) if a.mode == "reject" else None
    m = dr & real
    cen["leave_share"]["dR"] = dict(below=float(lo[m].sum() / total), above=float(hi[m].sum() / total))
    cen["leave_per_crossing"]["dR"] = float((lo[m] + hi[m]).sum() / nc[m].sum())
    cen["oob_share"]["dR_sum"] = float((lo[m] + hi[m]).sum() / rejected) if a.mode == "reject" else None
    bins_lo, bins_hi = np.zeros(10), np.zeros(10)
    for k in range(K):
        pos = np.minimum((10 * np.arange(N[k])) // N[k], 9)
        np.add.at(bins_lo, pos, lo[k, 7:P[k]])
        np.add.at(bins_hi, pos, hi[k, 7:P[k]])
    cen["dR_by_position"] = dict(below=[float(v / total) for v in bins_lo], above=[float(v / total) for v in bins_hi])
    rej = res.trial_oob == 1
    nl = res.n_left[rej]
    cen["n_left_hist"] = {"1": int((nl == 1).sum()), "2": int((nl == 2).sum()), "3": int((nl == 3).sum()),
                          "4-7": int(((nl >= 4) & (nl <= 7)).sum()), "8+": int((nl >= 8).sum()), "0": int((nl == 0).sum())}
    cen["exactly_one"] = float((nl == 1).sum() / max(nl.size, 1))
    cen["rejected_snooker_share"] = float((rej & (res.snooker == 1)).sum() / max(rej.sum(), 1))
    live = res.trial_oob != 2
    cen["crossing_mean"] = float(nc.sum() / live.sum())
    cen["n_left_mean_all_proposals"] = float(np.where(res.n_left < 0, 0, res.n_left).sum() / live.sum())
    near_lo = near_hi = cnt = 0
    for k in range(K):
        x = res.chain[sel][:, k * n_pop:(k + 1) * n_pop, 7:P[k]]
        near_lo += int((x < -29.0).sum())
        near_hi += int((x > 29.0).sum())
        cnt += x.size
    cen["near_wall"] = dict(below=near_lo / cnt, above=near_hi / cnt)
    out["census"] = cen
    whole = json.load(open(a.out)) if os.path.exists(a.out) else {}
    whole.setdefault("setup", dict(dataset=cl.name, n_cells=cl.n_cells, chains=a.chains, n_gen=a.gens, thin=a.thin, n_burn=burn,
                                   seed=0, note="one run per mode, HIP events; DESIGN.md 7p's run with the census on"))
    whole[a.mode] = out
    json.dump(whole, open(a.out, "w"), indent=1)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("reject", "reflect"), required=True)
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--gens", type=int, default=16000)
    ap.add_argument("--thin", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(HERE, "bounds_census.json"))
    run(ap.parse_args())


if __name__ == "__main__":
    main()
