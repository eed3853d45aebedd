"""tci_mex('loocheck', ...) and options.stack of tci_mex('dram', ...) through the stand-in MATLAB API: the argument
checks (CPU; they come before the handle is touched) and, on the GPU, the outputs against Likelihood.loocheck bit for
bit, with MATLAB's conventions: X is P x S x n and s2 S x n column-major, cells and groups are 1-based (group 0 = none),
the pointwise arrays are N_max x 2 x n."""
import numpy as np
import pytest

from mexharness import MxPtr
from test_mex_gateway import _opts, data_struct, expect, mex  # noqa: F401  (mex: the module's gateway fixture)
from test_predict_mex import nd_double

PT = (("elpd_loo", "elpd_loo_i"), ("lppd", "lppd_i"), ("p_loo", "p_loo_i"), ("khat", "khat_i"))


def test_loocheck_arguments_are_checked(mex):
    fake = MxPtr(mex, mex.handle(12345))
    X = nd_double(mex, np.zeros((130, 40, 2)))
    cells12 = np.array([1.0, 2.0])
    s2 = np.ones((40, 2))
    try:
        expect("tci:handle", mex.call, "loocheck", fake, cells12, X, s2, nlhs=2)            # only the handle is bad
        expect("tci:handle", mex.call, "loocheck", fake, cells12, X, s2, np.array([1.0, 2.0]), nlhs=2)
        expect("tci:handle", mex.call, "loocheck", fake, cells12, X, s2, np.zeros(0), _opts(mex, tol=1e-9, max_iter=10.0))
        expect("tci:arg", mex.call, "loocheck", fake, cells12, X)                           # too few arguments
        expect("tci:arg", mex.call, "loocheck", fake, cells12, X, s2, np.zeros(0), _opts(mex, tol=0.0), 1.0)  # too many
        expect("tci:arg", mex.call, "loocheck", fake, np.array([1.0, 2.0, 3.0]), X, s2)     # n differs from X's pages
        expect("tci:arg", mex.call, "loocheck", fake, np.array([0.0, 1.0]), X, s2)          # cells are 1-based
        expect("tci:arg", mex.call, "loocheck", fake, cells12, X, np.ones((40, 3)))         # s2 is S x n
        expect("tci:arg", mex.call, "loocheck", fake, cells12, X, np.ones((2, 40)))
        b = s2.copy()
        b[3, 1] = np.nan
        assert "s2(44)" in expect("tci:arg", mex.call, "loocheck", fake, cells12, X, b).msg  # column-major, 1-based
        expect("tci:arg", mex.call, "loocheck", fake, cells12, X, s2, np.array([1.0, 1.0]))  # one group, two cells
        expect("tci:arg", mex.call, "loocheck", fake, cells12, X, s2, np.array([1.0, 3.0]))  # group in [0, n]
        expect("tci:arg", mex.call, "loocheck", fake, cells12, X, s2, np.array([1.0]))
        expect("tci:opts", mex.call, "loocheck", fake, cells12, X, s2, np.zeros(0), _opts(mex, levels=1.0))
        expect("tci:opts", mex.call, "loocheck", fake, cells12, X, s2, np.zeros(0), _opts(mex, khat_threshold=0.0))
        expect("tci:opts", mex.call, "loocheck", fake, cells12, X, s2, np.zeros(0), _opts(mex, max_iter=0.0))
        expect("tci:opts", mex.call, "loocheck", fake, cells12, X, s2, np.zeros(0), _opts(mex, tol=-1.0))
        for S in (31, 4097):
            bad = nd_double(mex, np.zeros((9, S, 2)))
            expect("tci:arg", mex.call, "loocheck", fake, cells12, bad, np.ones((S, 2)))
            bad.free()
    finally:
        X.free()
        fake.free()


@pytest.mark.gpu
def test_loocheck_equals_the_binding_bitwise(mex, cells):
    from transcriptioncycleinference_amd import Likelihood
    from transcriptioncycleinference_amd.data import draw_x0

    d = data_struct(mex, cells, range(cells.n_cells))
    h = mex.call("create", d, "P2P-MS2v5-LacZ-PP7v4", 0.0)[0]
    d.free()
    gw = MxPtr(mex, mex.handle(int(h[0, 0])))
    rng = np.random.default_rng(23)
    cid = np.array([298, 0, 298, 42, 0], np.int32)
    group = np.array([1, 0, 1, -1, 0], np.int32)
    S, P = 70, 7 + int(cells.lengths.max())
    theta = np.zeros((len(cid), S, P))
    for k, c in enumerate(cid):
        for s in range(S):
            r = draw_x0(rng, int(cells.lengths[c]))
            theta[k, s, :len(r)] = r
    s2 = rng.uniform(5.0, 20.0, (len(cid), S))
    X = nd_double(mex, np.transpose(theta, (2, 1, 0)))     # P x S x n
    one = (cid + 1).astype(np.float64)
    try:
        with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
            for grp, opts, kw in ((group, None, {}), (None, None, {}),
                                  (group, {"khat_threshold": 0.5, "max_iter": 7.0, "tol": 0.0},
                                   dict(khat_threshold=0.5, max_iter=7, tol=0.0))):
                args = [s2.T]
                if grp is not None or opts is not None:
                    args.append(np.zeros(0) if grp is None else (grp + 1).astype(np.float64))
                if opts is not None:
                    args.append(_opts(mex, **opts))
                pt, ch = mex.call("loocheck", gw, one, X, *args, nlhs=2)
                want = lk.loocheck(theta, s2, cid, group=grp, **kw)
                nmax = int(cells.lengths[cid].max())
                assert list(pt) == [a for a, _ in PT]
                for f, w in PT:
                    assert pt[f].shape == (nmax, 2, len(cid))
                    assert np.transpose(pt[f], (2, 1, 0)).tobytes() == getattr(want, w).tobytes(), f
                for f in ("elpd_loo", "p_loo", "lppd", "khat_max", "weight"):
                    assert ch[f].shape == (1, len(cid)) and ch[f][0].tobytes() == getattr(want, f).tobytes(), f
                assert ch["n_obs"][0].tolist() == want.n_obs.tolist()
                assert ch["n_khat_bad"][0].tolist() == want.n_khat_bad.tolist()
                ng = 0 if grp is None else 2
                assert ch["elpd_stack"].size == ng == want.elpd_stack.size
                if ng:
                    assert ch["elpd_stack"][0].tobytes() == want.elpd_stack.tobytes()
                    assert ch["n_points"][0].tolist() == want.n_points.tolist()
                    assert ch["n_iter"][0].tolist() == want.n_iter.tolist()
                assert ch["khat_threshold"][0, 0] == want.khat_threshold and ch["kernel_ms"][0, 0] > 0
            assert want.n_iter.max() == 7
        expect("tci:call", mex.call, "loocheck", gw, np.array([300.0, 1.0, 2.0, 3.0, 4.0]), X, s2.T)   # cell 300 of 299
    finally:
        X.free()
        mex.call("destroy", gw, nlhs=0)
        gw.free()


@pytest.mark.gpu
def test_dram_stack_equals_loocheck_on_the_kept_rows(mex, cells):
    """options.stack of 'dram': two chains of one cell and one of another; res.stack is Likelihood.loocheck on the rows
    it names, and everything else of the run is that of the same call without the option."""
    from transcriptioncycleinference_amd import Likelihood, mcmc

    ids = np.array([0, 150, 0], np.int32)
    d = data_struct(mex, cells, range(cells.n_cells))
    h = mex.call("create", d, "P2P-MS2v5-LacZ-PP7v4", 0.0)[0]
    d.free()
    gw = MxPtr(mex, mex.handle(int(h[0, 0])))
    plan = mcmc.plan_fit(cells, [0, 150], 5, replicates=2)
    pick = [0, 1, 2]                                           # (cell 0, r 0), (cell 150, r 0), (cell 0, r 1)
    T = lambda a: np.ascontiguousarray(a[pick].T)  # noqa: E731   P x n
    opts = {"nsimu": 900.0, "burnintime": 400.0, "thin": 4.0, "seed": 11.0, "chain_keys": np.array([0.0, 150.0, 7.0])}
    args = ((ids + 1).astype(np.float64), T(plan.x0), T(plan.lower), T(plan.upper), T(plan.prior_mu), T(plan.prior_sig),
            T(plan.qcov_diag), 1.0)
    try:
        base, chain, s2c = mex.call("dram", gw, *args, _opts(mex, **opts), nlhs=3)
        res, chain2, s2c2 = mex.call("dram", gw, *args, _opts(mex, **{**opts, "stack": 64.0}), nlhs=3)
        only = mex.call("dram", gw, *args, _opts(mex, **{**opts, "stack": 64.0}), nlhs=1)[0]     # no chain output asked for
        assert "stack" not in base and chain.tobytes() == chain2.tobytes() and s2c.tobytes() == s2c2.tobytes()
        for f in ("mean", "std", "final_theta", "sigma_mean", "accept_rate"):
            assert base[f].tobytes() == res[f].tobytes() == only[f].tobytes(), f
        st = res["stack"]
        n_keep = chain.shape[2]
        k0 = (400 - 1 + 4 - 1) // 4
        rows = n_keep - k0
        idx = mcmc.predict_rows(rows, 64)
        assert (st["rows"][0] - 1).astype(np.int64).tolist() == idx.tolist() and st["group"][0].tolist() == [1, 2, 1]
        theta = np.ascontiguousarray(np.transpose(chain[:, :, k0:][:, :, idx], (1, 2, 0)))    # n x S x P
        s2 = np.ascontiguousarray(s2c[:, k0:][:, idx])
        with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
            want = lk.loocheck(theta, s2, ids, group=np.array([0, 1, 0], np.int32))
        for s in (st, only["stack"]):
            for f in ("elpd_loo_i", "lppd_i", "p_loo_i", "khat_i"):
                assert np.transpose(s[f], (2, 1, 0)).tobytes() == getattr(want, f).tobytes(), f
            for f in ("elpd_loo", "p_loo", "lppd", "khat_max", "weight"):
                assert s[f][0].tobytes() == getattr(want, f).tobytes(), f
            assert s["elpd_stack"][0].tobytes() == want.elpd_stack.tobytes()
            assert s["n_khat_bad"][0].tolist() == want.n_khat_bad.tolist() and s["weight"][0, 1] == 1.0
        expect("tci:opts", mex.call, "dram", gw, *args, _opts(mex, **{**opts, "stack": 16.0}))
        expect("tci:opts", mex.call, "dram", gw, *args, _opts(mex, **{**opts, "stack": 64.0, "thin": 0.0}))
        expect("tci:opts", mex.call, "dram", gw, *args, _opts(mex, **{**opts, "stack": 64.0, "nsimu": 500.0}))   # 25 kept rows
    finally:
        mex.call("destroy", gw, nlhs=0)
        gw.free()
