"""tci_mex('demczs', ...) with the options bounds and census through the stand-in MATLAB API: the option checks that
come before the handle is touched (CPU) and, on the GPU, bitwise equality of the new fields with the Python binding in
MATLAB's conventions: n_cross, oob_lo, oob_hi and orient come back P x n_pop x n (as pop), n_left and n_refl
n_chains x rows (as the other logs), n_reflected n_pop x n."""
import numpy as np
import pytest

from mexharness import MxPtr
from test_demczs_mex import IDS, M0, N_GEN, N_POP, SEED, zs_args
from test_mex_gateway import _opts, data_struct, expect, mex  # noqa: F401  (mex: the gateway fixture)

CENSUS = ("n_cross", "oob_lo", "oob_hi", "n_left")
REFLECT = ("n_refl", "n_reflected", "orient")


def test_bounds_and_census_options_are_checked(mex, cells):
    fake = MxPtr(mex, mex.handle(12345))
    _, _, a = zs_args(cells)
    for ident, kv, word in (("tci:opts", {"bounds": "fold"}, "bounds"), ("tci:opts", {"bounds": 1.0}, "bounds"),
                            ("tci:opts", {"census": 2.0}, "census"), ("tci:opts", {"census": 0.5}, "census"),
                            ("tci:handle", {"bounds": "reflect", "census": 1.0}, ""),     # well-formed: only the handle is bad
                            ("tci:handle", {"bounds": "reject", "census": 0.0}, "")):
        o = _opts(mex, **kv)
        e = expect(ident, mex.call, "demczs", fake, *a, 1.0, o)
        assert word in e.msg, (kv, e.msg)
        o.free()
    for kv in ({"bounds": "reflect"}, {"census": 1.0}):                                    # options of 'demczs' alone
        o = _opts(mex, **kv)
        e = expect("tci:opts", mex.call, "demc", fake, *a[:2], *a[3:], 1.0, o)
        assert list(kv)[0] in e.msg
        o.free()
    fake.free()


@pytest.mark.gpu
def test_bounds_fields_equal_the_binding_bitwise(mex, cells):
    from transcriptioncycleinference_amd import Likelihood

    ds = data_struct(mex, cells, range(cells.n_cells))
    h = mex.call("create", ds, "P2P-MS2v5-LacZ-PP7v4", 0.0)[0]
    ds.free()
    gw = MxPtr(mex, mex.handle(int(h[0, 0])))
    sp, jit, a = zs_args(cells)
    K, P = len(IDS), sp.pop0.shape[2]
    B = K * N_POP
    # boxes drawn in around the starting rows, so that coordinates leave at both walls
    lo0, up0 = sp.pop0.min(axis=1), sp.pop0.max(axis=1)
    lo, up = np.maximum(sp.lower, lo0 - 0.25 * (up0 - lo0)), np.minimum(sp.upper, up0 + 0.25 * (up0 - lo0))
    a = a[:3] + [lo.T.copy(), up.T.copy()] + a[5:]
    kw = dict(thin=2, jump_every=2, CR=0.4, log_rows=5, append_every=2, p_snooker=0.3)
    try:
        with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
            cid = np.asarray(sp.cells, np.int32)
            run = lambda **k: lk.demczs(sp.pop0[:, :N_POP], sp.pop0, cid, lo, up, sp.prior_mu, sp.prior_sig, jit,  # noqa: E731
                                        n_gen=N_GEN, seed=SEED, updatesigma=False, **kw, **k)
            for bounds, census in (("reflect", True), ("reject", True), ("reflect", False), ("reject", False)):
                o = _opts(mex, n_gen=float(N_GEN), seed=float(SEED), updatesigma=0.0, bounds=bounds, census=float(census),
                          **{k: float(v) for k, v in kw.items()})
                got = mex.call("demczs", gw, *a, 1.0, o)[0]
                o.free()
                want = run(bounds=bounds, census=census)
                np.testing.assert_array_equal(np.transpose(got["chain"], (2, 1, 0)), want.chain)
                for f in ("logr", "accepted", "trial_oob", "snooker"):
                    np.testing.assert_array_equal(got[f].T, getattr(want, f), err_msg=f)
                on = (CENSUS if census else ()) + (REFLECT if bounds == "reflect" else ())
                assert all((f in got) == (f in on) for f in CENSUS + REFLECT), sorted(got)
                for f in on:
                    w = getattr(want, f)
                    if f in ("n_left", "n_refl"):
                        assert got[f].shape == (B, 5)
                        np.testing.assert_array_equal(got[f].T, w, err_msg=f)
                    elif f == "n_reflected":
                        np.testing.assert_array_equal(got[f].T, w, err_msg=f)
                    else:
                        assert got[f].shape == (P, N_POP, K)
                        np.testing.assert_array_equal(np.transpose(got[f], (2, 1, 0)), w, err_msg=f)
                if census:
                    assert want.oob_lo.clip(0).sum() > 0 and want.oob_hi.clip(0).sum() > 0
                if bounds == "reflect":
                    assert want.n_refl.sum() > 0
    finally:
        mex.call("destroy", gw, nlhs=0)
        gw.free()
