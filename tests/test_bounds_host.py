"""The bounds census and the oriented reflection of DE-MC(zs), host side (no GPU): the restatement
(tests/bounds_oracle.py) with a synthetic SS. That the oriented rule leaves the uniform law on a box invariant and plain
reflection does not, that a reflected move is undone by its reverse, the census identities, and that reject mode is
tests/demczs_oracle.py bit for bit; then the defaults and the struct layouts of the C ABI."""
import ctypes as C

import numpy as np
import pytest

import bounds_oracle as B
import demczs_oracle as O

U = 2.0 ** -53


def flat_ss(rows):
    return np.ones(len(rows))


_flat = {}


def flat_run(oriented):
    if oriented not in _flat:
        T = B.FLAT
        pop0, z0, lo, up, mu, sig, jit = B.flat_box()
        _flat[oriented] = B.run(flat_ss, pop0, z0, 2, lo, up, mu, sig, jit, key=1, seed=T["seed"], n_gen=T["n_gen"],
                                thin=T["thin"], CR=T["CR"], append_every=T["n_gen"] + 1, p_snooker=0.0, mode=B.REFLECT,
                                oriented=oriented)
    return _flat[oriented]


def test_oriented_reflection_keeps_the_uniform_law_on_the_box():
    """B.FLAT: every in-box trial is accepted, so the chain is the proposal's own law. Measured on this run (seed 3):
    worst |z| 1.24 over the five statistics, least ESS 369, about 41 % of the proposals reflected."""
    T = B.FLAT
    r = flat_run(True)
    z, ess, vals = B.flat_stats(r["chain"][T["n_burn"]:])
    print(f"oriented: worst z {z:.3f}, least ESS {ess:.1f}, quadrants {vals[:4]}, E[xy] {vals[4]:.5f}, "
          f"{int((r['n_refl'] > 0).sum())} of {r['n_refl'].size} proposals reflected")
    assert r["archive"].shape[0] == T["m0"]                        # the kernel is fixed
    assert np.all(r["accepted"] == 1) and r["n_oob"].sum() == 0    # flat target, and no step beyond the width
    assert (r["n_refl"] > 0).mean() > 0.2 and r["orient"][:, :2].any() and not r["orient"][:, :2].all()
    assert np.all((r["chain"] >= 0) & (r["chain"] <= 1))
    assert z <= O.TARGET_Z


def test_plain_reflection_is_refused_by_the_same_statistic():
    """The cap on the test's own blindness: with the orientation dropped the (low, low) and (high, high) quadrants hold
    about twice their mass and the other two are nearly empty (count the preimages of x -> R(x +- d), d along (1, 1)).
    Measured: worst |z| 313, quadrant masses 0.47, 0.03, 0.03, 0.46."""
    T = B.FLAT
    r = flat_run(False)
    z, ess, vals = B.flat_stats(r["chain"][T["n_burn"]:])
    print(f"plain: worst z {z:.3f}, least ESS {ess:.1f}, quadrants {vals[:4]}, E[xy] {vals[4]:.5f}")
    assert np.all(r["accepted"] == 1) and not r["orient"].any()
    assert z > 10 * O.TARGET_Z
    assert vals[0] > 0.4 and vals[3] > 0.4 and vals[1] < 0.1 and vals[2] < 0.1


def unfolded(x, o, lo, w):
    """The circle coordinate in [0, 2 w) of box coordinate x with orientation bit o."""
    return np.where(o.astype(bool), 2 * w - (x - lo), x - lo)


def walls(u, d, w):
    """Wall points (multiples of w) strictly inside the unfolded segment from u to u + d."""
    a, b = np.minimum(u, u + d), np.maximum(u, u + d)
    return (np.ceil(b / w) - 1 - np.floor(a / w)).astype(np.int64)


def test_a_reflected_move_is_undone_by_its_reverse():
    """Random (x, orient, d) on boxes of several places and widths. Forward: B.step with increment d (no jitter). When
    it needs at most one reflection, the reverse from the result with -d needs at most one too, returns the orientation
    bit exactly and x up to the roundings: either direction rounds an addition and, when it reflects, a subtraction
    and an addition or subtraction more, six operations on values of size at most S = |lower| + |upper| + |d|, each
    off by at most u S (u = 2^-53): 8 u S holds them. When the forward move needs two, so does the reverse, taken from
    the point the twice-folded segment ends at: the wall points inside the unfolded segment are the same set."""
    rs = np.random.default_rng(7)
    n = 200000
    lo = rs.choice([-30.0, 0.0, 4.2 - 1e-5, 0.3], n)
    w = np.where(lo == 4.2 - 1e-5, 2e-5, rs.choice([60.0, 1.0, 10.0], n))
    up = lo + w
    x = lo + w * rs.random(n)
    o = rs.integers(0, 2, n).astype(np.uint8)
    d = w * rs.normal(size=n) * rs.choice([0.05, 0.5, 1.0], n)
    zero = np.zeros(n)
    raw, t, ot, below, above, refl = B.step(x, o, d, zero, lo, up)
    still = ~((t >= lo) & (t <= up))
    S = np.abs(lo) + np.abs(up) + np.abs(d)
    # the count of wall points the unfolded segment crosses decides: none, one reflection, or a rejection
    u0 = unfolded(x, o, lo, w)
    k = walls(u0, d, w)
    edge = np.abs((u0 + d) / w - np.round((u0 + d) / w)) < 1e-9      # an end within rounding of a wall: either count
    np.testing.assert_array_equal(refl[~edge], k[~edge] >= 1)
    np.testing.assert_array_equal(still[~edge], k[~edge] >= 2)
    assert (k == 0).sum() > n // 10 and (k == 1).sum() > n // 10 and (k >= 2).sum() > n // 100
    assert below.sum() > n // 20 and above.sum() > n // 20
    one = ~still & ~edge
    _, back, ob, _, _, refl_b = B.step(t[one], ot[one], -d[one], zero[one], lo[one], up[one])
    assert np.all((back >= lo[one]) & (back <= up[one]))               # the reverse needs at most one reflection as well
    np.testing.assert_array_equal(refl_b, refl[one])                   # and exactly when the forward move did
    np.testing.assert_array_equal(ob, o[one])
    worst = np.max(np.abs(back - x[one]) / (U * S[one]))
    print(f"reverse move: worst |x' - x| = {worst:.2f} u S")
    assert worst <= 8.0
    # two reflections: the reverse from the segment's far end crosses the same wall points
    two = still & ~edge
    u1 = np.mod(u0[two] + d[two], 2 * w[two])
    np.testing.assert_array_equal(walls(u1, -d[two], w[two]), k[two])
    # a NaN trial is left alone by the reflection and stays outside
    raw, t, ot, below, above, refl = B.step(np.array([0.5]), np.array([1], np.uint8), np.array([np.nan]), np.zeros(1), 0.0, 1.0)
    assert np.isnan(t[0]) and not below[0] and not above[0] and not refl[0] and ot[0] == 1


def tight_run(mode, p_snooker=0.5, **kw):
    """A 12-coordinate Gaussian inside bounds at mu +- 1.2 sig: tight enough for both walls to be met often."""
    T = {**O.SMALL, "n_pop": 16, "m0": 40, "n_gen": 60, "thin": 1, **kw}
    P = T["P"]
    pop0, z0, lo, up, mu, sig = O.gaussian_target(P, T["n_pop"], T["m0"], T["pop_seed"])
    lo, up = mu - 1.2 * sig, mu + 1.2 * sig
    pop0, z0 = np.clip(pop0, lo, up), np.clip(z0, lo, up)
    pad = lambda a, v: np.concatenate([a, np.full(a.shape[:-1] + (3,), v)], axis=-1)  # noqa: E731  ld = P + 3
    args = (flat_ss, pad(pop0, 7.0), pad(z0, 9.0), P, pad(lo, -np.inf), pad(up, np.inf), pad(mu, 0.0), pad(sig, np.inf),
            pad(0.05 * sig, 0.0))
    kw = dict(sigma2_0=T["sigma2_0"], key=290, seed=T["seed"], n_gen=T["n_gen"], thin=T["thin"], jump_every=4, CR=0.3,
              append_every=3, p_snooker=p_snooker)
    return args, kw, B.run(*args, mode=mode, **kw)


@pytest.mark.parametrize("mode", [B.REJECT, B.REFLECT])
def test_census_identities(mode):
    args, kw, r = tight_run(mode)
    P = args[3]
    nc, lo, hi, nl = r["n_cross"], r["oob_lo"], r["oob_hi"], r["n_left"]
    assert np.all(nc[:, P:] == -1) and np.all(lo[:, P:] == -1) and np.all(hi[:, P:] == -1)
    assert np.all(lo[:, :P] + hi[:, :P] <= nc[:, :P]) and np.all(lo[:, :P] >= 0) and np.all(hi[:, :P] >= 0)
    assert lo[:, :P].sum() > 0 and hi[:, :P].sum() > 0
    null = r["trial_oob"] == 2
    assert null.sum() > 0 and np.all(nl[null] == -1) and np.all(nl[~null] >= 0)
    np.testing.assert_array_equal(np.where(null, 0, nl).sum(axis=0), (lo[:, :P] + hi[:, :P]).sum(axis=1))
    # a snooker move crosses every coordinate, a jump generation too; a null move none
    snk, jump = r["snooker"] == 1, (np.arange(1, kw["n_gen"] + 1) % 4 == 0)[:, None]
    assert np.all(nc[:, :P].sum(axis=1) >= P * ((snk & ~null) | (~snk & jump)).sum(axis=0))
    assert np.all(nc[:, :P].sum(axis=1) <= P * (~null).sum(axis=0))
    if mode == B.REJECT:
        np.testing.assert_array_equal(nl > 0, r["trial_oob"] == 1)      # NaN-free inputs
        assert not r["n_refl"].any() and not r["orient"].any() and not r["n_reflected"].any()
    else:
        par = ~snk
        np.testing.assert_array_equal(r["n_refl"][par], nl[par])        # every leaving coordinate is reflected once
        assert not r["n_refl"][snk].any()
        assert np.all((r["trial_oob"] == 1)[par] <= (nl[par] > 0))      # a rejected parallel move overshot twice
        np.testing.assert_array_equal(r["n_reflected"], (par & (r["trial_oob"] == 0) & (r["n_refl"] > 0)).sum(axis=0))
        assert r["flips"].sum() > 0 and r["orient"][:, :P].any()
        assert not r["orient"][:, P:].any()
        x = r["chain"][:, :, :P]
        assert np.all((x >= args[4][:P]) & (x <= args[5][:P]))


@pytest.mark.parametrize("p_snooker", [0.0, 0.5])
def test_reject_mode_is_demczs_oracle_bit_for_bit(p_snooker):
    args, kw, r = tight_run(B.REJECT, p_snooker)
    want = O.run(*args, **kw)
    for f in ("chain", "s2chain", "sschain", "prichain", "pop", "ss", "pri", "n_oob", "n_null", "n_evals", "logr",
              "accepted", "trial_oob", "snooker", "ljac", "archive", "accept_rate"):
        np.testing.assert_array_equal(r[f], want[f], err_msg=f)
    assert r["n_oob"].sum() > 0 and r["accepted"].sum() > 0
    # reflect mode with nothing leaving is reject mode: the same run inside bounds nothing reaches
    wide = list(args)
    wide[4], wide[5] = np.full_like(args[4], -1e6), np.full_like(args[5], 1e6)
    a, b = B.run(*wide, mode=B.REJECT, **kw), B.run(*wide, mode=B.REFLECT, **kw)
    for f in ("chain", "logr", "accepted", "trial_oob", "archive", "n_cross", "oob_lo", "oob_hi", "n_left"):
        np.testing.assert_array_equal(a[f], b[f], err_msg=f)
    assert not b["n_refl"].any() and not b["orient"].any() and not a["oob_lo"][:, :args[3]].any()


@pytest.fixture(scope="module")
def lib():
    from transcriptioncycleinference_amd import _lib
    from transcriptioncycleinference_amd.build import build_library

    build_library()
    return _lib.load()


def test_defaults_struct_layouts_and_the_bindings_own_refusals(lib):
    from transcriptioncycleinference_amd import Likelihood, _lib, likelihood, mcmc

    o = _lib.tci_bounds_options(7, 7, 7)
    assert lib.tci_bounds_defaults(C.byref(o)) == _lib.TCI_OK and (o.mode, o.census, o.flags) == (0, 0, 0)
    assert lib.tci_bounds_defaults(None) == _lib.TCI_EINVAL
    assert (_lib.TCI_BOUNDS_REJECT, _lib.TCI_BOUNDS_REFLECT) == (0, 1)
    assert C.sizeof(_lib.tci_bounds_options) == 16 and C.sizeof(_lib.tci_bounds_outputs) == 56
    assert [f for f, _ in _lib.tci_bounds_outputs._fields_] == ["n_cross", "oob_lo", "oob_hi", "n_left", "n_refl",
                                                                "n_reflected", "orient"]
    assert lib.tci_demczs_run_bounds(*([None] * 4), 0, None, 0, 0, 0, *([None] * 15)) == _lib.TCI_EINVAL
    for kw in (dict(bounds="fold"), dict(census=1)):
        with pytest.raises(ValueError, match="bounds|census"):
            Likelihood.demczs(None, np.zeros((1, 1, 8)), np.zeros((1, 3, 8)), [0], *([np.zeros((1, 8))] * 5), **kw)
    assert {"bounds", "census"} <= set(mcmc.DEMCZS_KEYS) and not {"bounds", "census"} & set(mcmc.DEMC_KEYS)
    assert {"n_cross", "oob_lo", "oob_hi", "reflect_rate", "oob_share"} <= set(mcmc.DEMCZS_FIELDS)
    with pytest.raises(ValueError, match="bounds"):
        mcmc._demczs_arg(dict(bounds="fold"))
    assert mcmc._demczs_arg(dict(bounds="reflect", census=True)) == dict(n_pop=4, n_gen=1000, bounds="reflect", census=True)
    dz = likelihood.DemcZs.empty_zs(2, 3, 9, 4, 1, 4, 5, 2, False)
    out = dz.with_bounds("reflect", True)
    assert dz.n_cross.shape == dz.orient.shape == (2, 3, 9) and dz.n_left.shape == dz.n_refl.shape == (4, 6)
    assert out.n_cross and out.orient and dz.n_reflected.shape == (2, 3)
