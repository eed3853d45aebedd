"""tci_mex('chainstats', ...) and the fifth output of tci_mex('dram', ...) through the stand-in MATLAB
API: argument checks (CPU; they come before the handle is touched) and, on the GPU, bitwise equality with
the Python binding, in MATLAB's conventions: chain is P x n x rows, s2chain n x rows, statistics P x n."""
import numpy as np
import pytest

import chainstats_oracle as O
from mexharness import MxPtr
from test_mex_gateway import _dram_args, _opts, data_struct, expect, mex  # noqa: F401  (mex: the gateway fixture)
from test_predict_mex import nd_double

KEYS = ("mcerr", "tau", "tau_window", "geweke_z", "geweke_p")


def test_chainstats_arguments_are_checked(mex):
    fake = MxPtr(mex, mex.handle(12345))
    X = nd_double(mex, np.zeros((9, 2, 30)))
    s2 = np.zeros((2, 30))
    none = np.zeros((0, 0))
    try:
        expect("tci:handle", mex.call, "chainstats", fake, X, s2, np.array([9.0, 8.0]))        # only the handle is bad
        expect("tci:handle", mex.call, "chainstats", fake, X, none, none, 8.0)                 # [] s2chain, [] npar
        expect("tci:arg", mex.call, "chainstats", fake, X, s2)                                 # too few arguments
        expect("tci:arg", mex.call, "chainstats", fake, X, s2, none, 0.0, 1.0)                 # too many
        expect("tci:arg", mex.call, "chainstats", fake, X, np.zeros((2, 29)), none)            # s2chain: n x rows
        expect("tci:arg", mex.call, "chainstats", fake, X, np.zeros((30, 2)), none)
        expect("tci:arg", mex.call, "chainstats", fake, X, s2, np.array([9.0]))                # one npar per chain
        expect("tci:arg", mex.call, "chainstats", fake, X, s2, np.array([10.0, 1.0]))          # npar <= P
        expect("tci:arg", mex.call, "chainstats", fake, X, s2, np.array([1.5, 1.0]))
        expect("tci:arg", mex.call, "chainstats", fake, X, s2, none, -1.0)                     # max_lag >= 0
        expect("tci:arg", mex.call, "chainstats", fake, X, s2, none, 2.5)
        lg = MxPtr(mex, mex.logical([True, False]))
        expect("tci:arg", mex.call, "chainstats", fake, lg, none, none)                        # chain must be double
        lg.free()
        bad = nd_double(mex, np.zeros((9, 2, 30, 2)))
        expect("tci:arg", mex.call, "chainstats", fake, bad, none, none)
        bad.free()
    finally:
        X.free()
        fake.free()


@pytest.mark.gpu
def test_chainstats_and_dram_statistics_equal_the_binding_bitwise(mex, cells):
    from transcriptioncycleinference_amd import Likelihood
    from transcriptioncycleinference_amd.mcmc import DramOptions, dram_run

    d = data_struct(mex, cells, range(cells.n_cells))
    h = mex.call("create", d, "P2P-MS2v5-LacZ-PP7v4", 0.0)[0]
    d.free()
    gw = MxPtr(mex, mex.handle(int(h[0, 0])))
    rows, n, P = 257, 3, 65
    x = O.ar1_columns(np.random.default_rng(7), rows, n * (P + 1))
    chain = np.ascontiguousarray(x[:, :n * P].reshape(rows, n, P))
    s2 = np.ascontiguousarray(x[:, n * P:])
    npar = np.array([65, 32, 62], np.int32)
    X = nd_double(mex, np.transpose(chain, (2, 1, 0)))       # P x n x rows
    try:
        with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
            for ml in (0, 8):
                got = mex.call("chainstats", gw, X, s2.T.copy(), npar.astype(np.float64), float(ml))[0]
                want = lk.chainstats(chain, s2, npar, max_lag=ml)
                for k in KEYS:
                    assert got[k].shape == (P, n) and got["s2_" + k].shape == (1, n)
                    assert got[k].T.astype(np.float64).tobytes() == getattr(want, k).astype(np.float64).tobytes(), k
                    assert got["s2_" + k][0].tobytes() == getattr(want, "s2_" + k).astype(np.float64).tobytes(), k
                assert got["n_rows"][0, 0] == rows
            bare = mex.call("chainstats", gw, X, np.zeros((0, 0)), np.zeros((0, 0)))[0]
            assert np.array_equal(bare["tau"].T, lk.chainstats(chain).tau) and np.all(bare["s2_tau_window"] == -1)
            # 'dram' with a fifth output: tci_dram_run_stats
            ids = [0, 150, 298]
            plan, a = _dram_args(mex, cells, ids)
            keys = np.asarray(plan.cells, np.int64)
            o = _opts(mex, nsimu=600.0, burnintime=200.0, adaptint=100.0, seed=5.0, max_lag=300.0,
                      chain_keys=keys.astype(np.float64))
            res, ch, s2c, R, st = mex.call("dram", gw, *a, o, nlhs=5)
            four = mex.call("dram", gw, *a, o, nlhs=4)
            o.free()
            do = DramOptions(n_steps=600, burnintime=200, adaptint=100, stats_from=200, thin=1, seed=5)
            w = dram_run(lk, np.asarray(plan.cells, np.int32), plan.x0, plan.lower, plan.upper, plan.prior_mu,
                         plan.prior_sig, plan.qcov_diag, 1.0, do, chain_keys=keys, stats=True, max_lag=300)
            assert st["n_rows"][0, 0] == 401 == w.stats.n_rows
            for k in KEYS:
                assert st[k].T.astype(np.float64).tobytes() == getattr(w.stats, k).astype(np.float64).tobytes(), k
                assert st["s2_" + k][0].tobytes() == getattr(w.stats, "s2_" + k).astype(np.float64).tobytes(), k
            assert np.array_equal(np.transpose(ch, (2, 1, 0)), w.chain)
            assert four[1].tobytes() == ch.tobytes() and four[0]["mean"].tobytes() == res["mean"].tobytes()
    finally:
        X.free()
        mex.call("destroy", gw, nlhs=0)
        gw.free()
