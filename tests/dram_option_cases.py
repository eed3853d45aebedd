"""Cases of the sampler's option space for the comparison with the CPU restatement -- host only.

tests/test_dram_options_gpu.py runs every (group, case) on the GPU and compares it with the restatement's
chains (oracle/tci_dram_oracle.c); tests/test_oracle_dram_options.py asserts on the restatement alone that
every case reaches the branch it is named for. Both read the same cells, inputs and restatement outputs
from here, computed once per (group, case).

Cells: the synthetic generator of test_dram_gpu._restatement_case (data.synthetic_cells, two cells per
length), with the noise-free signal evaluated by the C oracle's forward model on the interpolation grid
and not by the GPU's, so that a machine without a GPU builds bit for bit the cells the GPU test runs on.
"""
import dataclasses

import numpy as np

# group -> (cells per length, points per cell, data seed)
GROUPS = {
    "small": (2, (9, 40), 20201050),  # P = 16 and 47 under one ld: RPL = 1, a chain shorter than ld
    "mid": (2, (150,), 20201051),     # P = 157: RPL = 4, k_adapt_mfma<8, 13, 12>
    "gt": (2, (210,), 20201052),      # P = 217: RPL = 4, k_adapt_gt
}
# group -> (largest P, rows per lane of the context, the adaptation kernel dram_launch_adapt picks)
GROUP_EXPECT = {"small": (47, 1, "mfma<8,9,6,4>"), "mid": (157, 4, "mfma<8,13,12>"), "gt": (217, 4, "gt")}
CASES = ("am", "fixed_sigma", "scales", "burnin_up", "burnin_only", "no_adapt", "ragged", "burnin_zero", "priors",
         "hierarchical", "tight_box", "frozen")
PLAN_SEED = 5
BASE = dict(n_steps=500, burnintime=300, adaptint=100, stats_from=200, thin=1, seed=91)
FIXED_SIGMA2 = (0.5, 2.0, 4.0, 0.25)   # per chain, none at the default 1
BURNIN_UP_QCOV = 1e-8                  # burnin_up: qcov_diag times this (proposal sd times 1e-4)
TIGHT_BOX_C = 1.0                      # tight_box: x0 +- c sqrt(qcov_diag) on v, tau and one rate
TIGHT_BOX_COORDS = (0, 1, 7 + 3)
FROZEN_COORD = 1                       # frozen: lower == upper == theta0 on tau
PRIOR_CORE_WIDTH = 1.0                 # priors: prior_sig = 1 sqrt(qcov_diag) on the seven core parameters
PRIOR_RATE = (2.0, 5.0)                # priors: N(2, 5) on the rates

_cells = {}
_cases = {}


@dataclasses.dataclass
class Case:
    group: str
    name: str
    cells: object
    construct: object
    cell_id: np.ndarray
    keys: np.ndarray
    theta0: np.ndarray
    lower: np.ndarray
    upper: np.ndarray
    prior_mu: np.ndarray
    prior_sig: np.ndarray
    qcov_diag: np.ndarray
    sigma2_0: object
    opts: object
    n: np.ndarray = None      # points per chain's cell
    want: dict = None         # the restatement's outputs (chain, s2chain, R, dr_counts, summaries)

    def run_restatement(self, c_oracle, **replace):
        """The restatement on this case's inputs, any of them replaced."""
        a = dict(theta0=self.theta0, lower=self.lower, upper=self.upper, prior_mu=self.prior_mu,
                 prior_sig=self.prior_sig, qcov_diag=self.qcov_diag, sigma2_0=self.sigma2_0, opts=self.opts)
        a.update(replace)
        return c_oracle.dram_run(self.cells, self.construct, self.cell_id, a["theta0"], a["lower"], a["upper"],
                                 a["prior_mu"], a["prior_sig"], a["qcov_diag"], a["sigma2_0"], a["opts"], keys=self.keys,
                                 want_chain=True, want_R=True, want_counts=True)


def group_cells(group, c_oracle):
    """(cells, construct) of the group."""
    if group in _cells:
        return _cells[group]
    from transcriptioncycleinference_amd import from_lists
    from transcriptioncycleinference_amd.construct import builtin_construct
    from transcriptioncycleinference_amd.data import synthetic_cells

    n_cells, n_points, seed = GROUPS[group]
    cs = builtin_construct("P2P-MS2v5-LacZ-PP7v4")

    def fwd(times, theta):
        m = np.zeros((len(times), max(len(t) for t in times)))
        p = np.zeros_like(m)
        for c, t in enumerate(times):
            m[c, :len(t)], p[c, :len(t)] = c_oracle.forward(t, cs, theta[c, :7 + len(t)], mode=1)
        return m, p

    parts = []
    for i, npts in enumerate(n_points):
        cc, _ = synthetic_cells(n_cells, npts, seed + 7919 * i, fwd)
        o = cc.offsets
        parts += [(cc.t[o[k]:o[k + 1]], cc.ms2[o[k]:o[k + 1]], cc.pp7[o[k]:o[k + 1]]) for k in range(n_cells)]
    _cells[group] = (from_lists(parts, f"synthetic-options-{group}"), cs)
    return _cells[group]


def hierarchical_v0(n_cells):
    """A previous fit's elongation rate per cell, inside (0, 10)."""
    return [2.0 + 1.375 * k for k in range(n_cells)]


def build(group, name, c_oracle):
    """The case's inputs and the restatement's outputs, computed once."""
    if (group, name) in _cases:
        return _cases[(group, name)]
    from transcriptioncycleinference_amd.mcmc import DramOptions, plan_fit

    cells, cs = group_cells(group, c_oracle)
    ids = list(range(len(cells.lengths)))
    v0 = hierarchical_v0(len(ids)) if name == "hierarchical" else None
    plan = plan_fit(cells, ids, PLAN_SEED, v0=v0)
    assert plan.cells == ids
    n = np.asarray(cells.lengths)[ids]
    x0, lo, hi, mu, sig, qd = (a.copy() for a in (plan.x0, plan.lower, plan.upper, plan.prior_mu, plan.prior_sig,
                                                  plan.qcov_diag))
    o, s20 = dict(BASE), 1.0
    if name == "baseline":
        pass
    elif name == "am":
        o.update(ntry=1)
    elif name == "fixed_sigma":
        o.update(updatesigma=False)
        s20 = np.array([FIXED_SIGMA2[k % len(FIXED_SIGMA2)] for k in range(len(ids))])
    elif name == "scales":
        o.update(drscale=3.0, adascale=0.7, qcovadj=1e-3, burnin_scale=4.0)
    elif name == "burnin_up":
        o.update(burnintime=400)
        qd *= BURNIN_UP_QCOV
    elif name == "burnin_only":
        o.update(burnintime=600)
    elif name == "no_adapt":
        o.update(adaptint=0)
    elif name == "ragged":
        o.update(adaptint=64, burnintime=150, n_steps=333, stats_from=77, thin=5)
    elif name == "burnin_zero":
        o.update(burnintime=0)
    elif name == "priors":
        for k in range(len(ids)):
            P = 7 + int(n[k])
            sig[k, :7] = PRIOR_CORE_WIDTH * np.sqrt(qd[k, :7])
            mu[k, :7] = x0[k, :7] + sig[k, :7] * np.where(np.arange(7) % 2 == 0, 1.0, -1.0)
            mu[k, 7:P], sig[k, 7:P] = PRIOR_RATE
    elif name == "hierarchical":
        pass
    elif name == "tight_box":
        for k in range(len(ids)):
            for j in TIGHT_BOX_COORDS:
                w = TIGHT_BOX_C * np.sqrt(qd[k, j])
                lo[k, j], hi[k, j] = max(lo[k, j], x0[k, j] - w), min(hi[k, j], x0[k, j] + w)
    elif name == "frozen":
        o.update(qcovadj=0.0)
        for k in range(len(ids)):
            P = 7 + int(n[k])
            x0[k, :P] = np.round(x0[k, :P] * 1024.0) / 1024.0
            lo[k, FROZEN_COORD] = hi[k, FROZEN_COORD] = x0[k, FROZEN_COORD]
            assert np.all(x0[k, :P] >= lo[k, :P]) and np.all(x0[k, :P] <= hi[k, :P])
    else:
        raise KeyError(name)
    case = Case(group, name, cells, cs, np.array(ids, np.int32), np.array(ids, np.int64), x0, lo, hi, mu, sig, qd, s20,
                DramOptions(**o), n)
    case.want = case.run_restatement(c_oracle)
    _cases[(group, name)] = case
    return case


def moved_mask(rows):
    """[n_rows - 1] per chain row 2..: the row differs from the one before (an accepted proposal)."""
    return np.any(rows[1:] != rows[:-1], axis=1)


def window_rejection_rates(case, k):
    """The restatement's rejection rate (rejected steps / adaptint) of chain k's every whole window, as
    run_chain counts it: steps are rows 2.., a window ends on a multiple of adaptint."""
    ai = int(case.opts.adaptint)
    assert int(case.opts.thin) == 1 and ai > 0
    P = 7 + int(case.n[k])
    rej = ~moved_mask(case.want["chain"][:, k, :P])  # rej[r - 2]: row r
    return np.array([rej[max(w * ai - 1, 0):(w + 1) * ai - 1].sum() / ai
                     for w in range(int(case.opts.n_steps) // ai)])


def burnin_windows(case):
    """How many windows end on a row before burnintime (those only scale R)."""
    ai, bt, ns = int(case.opts.adaptint), int(case.opts.burnintime), int(case.opts.n_steps)
    return sum(1 for row in range(ai, ns + 1, ai) if row < bt)
