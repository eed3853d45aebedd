"""Chain diagnostics on the device (tci_chainstats.hip) against the numpy oracle of
tests/chainstats_oracle.py: tau_window exactly, tau within 1e-9 relative, mcerr within 1e-10 relative,
Geweke's z and p within 1e-10 of max(1, |value|). Before any comparison every fixture asserts, from the
oracle alone, that each column's running Sokal sum stays at least 1e-6 from zero up to and including its
crossing, so no column is excused for sitting on a window boundary.

Largest errors seen on an MI355X over every case below: see DESIGN.md (chain diagnostics)."""
import math

import numpy as np
import pytest

import chainstats_oracle as O

pytestmark = pytest.mark.gpu

IDS = [0, 150, 298]   # three TestData cells of unequal length


@pytest.fixture(scope="module")
def lk(cells):
    from transcriptioncycleinference_amd import Likelihood

    with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as L:
        yield L


def ar_case(rows, n_chains, ld):
    """AR(1) chain + s2 chain (seeded), unequal npar over the chains, and the oracle's table."""
    rng = np.random.default_rng(7)
    x = O.ar1_columns(rng, rows, n_chains * (ld + 1))
    chain = np.ascontiguousarray(x[:, :n_chains * ld].reshape(rows, n_chains, ld))
    s2 = np.ascontiguousarray(x[:, n_chains * ld:])
    npar = np.array([ld, ld // 2, max(ld - 3, 1)][:n_chains], np.int32)
    want = O.table(chain, s2, npar)
    assert want["margin"] >= 1e-6, want["margin"]
    return chain, s2, npar, want


@pytest.mark.parametrize("ld", [1, 63, 64, 65, 136])
@pytest.mark.parametrize("rows", [19, 20, 21, 199, 200, 257, 1000])
def test_shape_edges_against_the_oracle(lk, rows, ld):
    for n_chains in (1, 3):
        chain, s2, npar, want = ar_case(rows, n_chains, ld)
        st = lk.chainstats(chain, s2, npar)
        assert st.n_rows == rows
        O.check(st, want, f"rows={rows} ld={ld} chains={n_chains} ")
        # what each row count is there for
        real = np.arange(ld)[None, :] < npar[:, None]
        assert np.all(np.isfinite(st.tau[real])) and np.all(st.tau_window[real] >= 1)
        assert np.all(np.isnan(st.tau[~real])) and np.all(st.tau_window[~real] == -1)   # padding
        assert np.all(np.isnan(st.mcerr[real])) == (rows < 20) and np.all(np.isnan(st.s2_mcerr)) == (rows < 20)
        assert np.all(np.isnan(st.geweke_z[real])) == (rows < 200) == np.all(np.isnan(st.geweke_p[real]))
        if rows >= 200:
            assert np.all(np.isfinite(st.geweke_z[real])) and np.all((st.geweke_p[real] >= 0) & (st.geweke_p[real] <= 1))
        if rows >= 257 and ld >= 4:
            assert st.tau_window[real].max() > 64     # the phi = 0.97 columns cross a 64-lag tile
        # without an s2 chain or npar: the s2 statistics are padding, every column is real
        if n_chains == 1 and ld == 65:
            bare = lk.chainstats(chain[:, 0, :])
            assert np.all(np.isnan(bare.s2_tau)) and np.all(bare.s2_tau_window == -1)
            assert bare.tau.tobytes() == st.tau.tobytes() and bare.geweke_p.tobytes() == st.geweke_p.tobytes()


def test_statistics_do_not_depend_on_the_layout(lk):
    """A column's bits depend on its values and n alone: not on ld, n_chains or where it sits."""
    chain, s2, _, _ = ar_case(257, 3, 65)
    full = lk.chainstats(chain, s2)
    one = lk.chainstats(np.ascontiguousarray(chain[:, 1:2, 3:40]), s2[:, 1:2])
    for k in ("mcerr", "tau", "tau_window", "geweke_z", "geweke_p"):
        assert getattr(one, k)[0].tobytes() == getattr(full, k)[1, 3:40].tobytes(), k
        assert getattr(one, "s2_" + k)[0].tobytes() == getattr(full, "s2_" + k)[1].tobytes(), k


def test_special_columns(lk):
    rows, ld = 257, 8
    x = O.ar1_columns(np.random.default_rng(7), rows, 4)
    chain = np.zeros((rows, 1, ld))
    chain[:, 0, 0] = x[:, 3]        # phi = 0.97
    chain[:, 0, 1] = 3.0            # constant
    chain[:, 0, 2] = x[:, 1]
    chain[100, 0, 2] = np.nan       # one NaN
    chain[:, 0, 3] = x[:, 2]
    chain[7, 0, 3] = np.inf         # one Inf
    chain[:, 0, 4] = 0.1            # a constant that is not a binary fraction
    chain[:, 0, 5] = x[:, 0]
    npar = np.array([6], np.int32)
    want = O.table(chain, None, npar)
    assert want["margin"] >= 1e-6 and want["tau_window"][0, 0] > 8
    st = lk.chainstats(chain, None, npar)
    O.check(st, want, "special ")
    for j in (1, 4):                # constant: tau = 0, window = 0, mcerr = 0, Geweke 0/0
        assert st.tau[0, j] == 0.0 and st.tau_window[0, j] == 0 and st.mcerr[0, j] == 0.0
        assert math.isnan(st.geweke_z[0, j]) and math.isnan(st.geweke_p[0, j])
    for j in (2, 3, 6, 7):          # a non-finite entry, and the padding: NaN everywhere
        assert all(math.isnan(a[0, j]) for a in (st.mcerr, st.tau, st.geweke_z, st.geweke_p)) and st.tau_window[0, j] == -1
    # max_lag = 8 on phi = 0.97: the window cannot close
    cap = lk.chainstats(chain, None, npar, max_lag=8)
    assert cap.tau[0, 0] == math.inf and cap.tau_window[0, 0] == 8
    O.check(cap, O.table(chain, None, npar, max_lag=8), "max_lag=8 ")
    # a cap past the crossing changes nothing; one past n is n
    for ml in (200, 10 ** 6):
        assert lk.chainstats(chain, None, npar, max_lag=ml).tau.tobytes() == st.tau.tobytes()


def test_bad_arguments_are_refused(lk):
    from transcriptioncycleinference_amd import TciError, _lib

    x = np.zeros((30, 2, 4))
    for kw in (dict(max_lag=-1), dict(npar=[5, 1]), dict(npar=[-1, 1])):
        with pytest.raises(TciError) as e:
            lk.chainstats(x, **kw)
        assert e.value.code == (_lib.TCI_EINVAL if "max_lag" in kw else _lib.TCI_ERANGE)
    with pytest.raises(TciError) as e:
        lk.chainstats(np.zeros((0, 2, 4)))
    assert e.value.code == _lib.TCI_EINVAL


# ---- tci_dram_run_stats: the statistics of the device chain ------------------------------------------

def _plan(lk):
    from transcriptioncycleinference_amd.mcmc import plan_fit

    p = plan_fit(lk.cells, IDS, 3)
    return (np.array(IDS, np.int32), p.x0, p.lower, p.upper, p.prior_mu, p.prior_sig, p.qcov_diag, 1.0)


def _opts(**kw):
    from transcriptioncycleinference_amd.mcmc import DramOptions

    return DramOptions(n_steps=2000, burnintime=500, adaptint=100, stats_from=500, thin=1, seed=19, **kw)


def _same(a, b):
    return all(getattr(a, k).tobytes() == getattr(b, k).tobytes() for k in
               ("mcerr", "tau", "tau_window", "geweke_z", "geweke_p", "s2_mcerr", "s2_tau", "s2_tau_window",
                "s2_geweke_z", "s2_geweke_p")) and a.n_rows == b.n_rows


@pytest.fixture(scope="module")
def dram(lk):
    from transcriptioncycleinference_amd.mcmc import dram_run

    return dram_run(lk, *_plan(lk), _opts(), stats=True)


def test_dram_statistics_equal_the_oracle_on_the_returned_chain(lk, dram):
    npar = (7 + lk.cells.lengths[IDS]).astype(np.int32)
    assert dram.stats.n_rows == 1501                                   # rows 500 .. 2000
    rows, s2 = dram.chain[499:], dram.s2chain[499:]
    want = O.table(rows, s2, npar)
    assert want["margin"] >= 1e-6, want["margin"]
    O.check(dram.stats, want, "dram ")
    # ... and equal, bit for bit, the statistics of the same rows handed back from the host
    assert _same(lk.chainstats(rows, s2, npar), dram.stats)


def test_dram_statistics_without_the_host_chain_and_plain_run(lk, dram):
    from transcriptioncycleinference_amd.mcmc import dram_run

    nochain = dram_run(lk, *_plan(lk), _opts(), stats=True, want_chain=False)
    assert nochain.chain is None and nochain.s2chain is None and _same(nochain.stats, dram.stats)
    plain = dram_run(lk, *_plan(lk), _opts())                          # tci_dram_run: nothing existing moved
    assert plain.stats is None
    assert plain.chain.tobytes() == dram.chain.tobytes() and plain.s2chain.tobytes() == dram.s2chain.tobytes()
    assert plain.mean.tobytes() == dram.mean.tobytes() and plain.std.tobytes() == dram.std.tobytes()


@pytest.mark.parametrize("engine", ["fused", "batched", "walk"])
def test_every_engine_gives_the_same_statistics(lk, dram, engine):
    from transcriptioncycleinference_amd.mcmc import dram_run

    res = dram_run(lk, *_plan(lk), _opts(engine=engine), stats=True, want_chain=False)
    assert _same(res.stats, dram.stats)


def test_dram_statistics_refusals(lk):
    from transcriptioncycleinference_amd import TciError, _lib
    from transcriptioncycleinference_amd.mcmc import DramOptions, dram_run

    for o, kw in ((DramOptions(n_steps=100, burnintime=50, stats_from=50, thin=0), {}),          # thin == 0
                  (DramOptions(n_steps=100, burnintime=50, stats_from=50, thin=1), dict(max_lag=-2)),
                  (DramOptions(n_steps=100, burnintime=50, stats_from=101, thin=1), {})):        # no row in range
        with pytest.raises(TciError) as e:
            dram_run(lk, *_plan(lk), o, stats=True, **kw)
        assert e.value.code == _lib.TCI_EINVAL
    # thinned: kept rows 1, 8, 15, ..; the first at or past row 50 is row 50 = 1 + 7 * 7
    o = DramOptions(n_steps=300, burnintime=100, stats_from=50, thin=7, seed=2)
    res = dram_run(lk, *_plan(lk), o, stats=True)
    assert res.stats.n_rows == 43 - 7
    npar = (7 + lk.cells.lengths[IDS]).astype(np.int32)
    assert _same(lk.chainstats(res.chain[7:], res.s2chain[7:], npar), res.stats)


# ---- fit(..., diagnostics=True) -------------------------------------------------------------------------

FIT = dict(n_steps=2000, n_burn=500, seed=4, thin=1)


@pytest.fixture(scope="module")
def fitted(lk):
    from transcriptioncycleinference_amd.mcmc import fit

    return fit(lk, cells=IDS, diagnostics=True, **FIT)


def _diag_equal(a, b):
    from transcriptioncycleinference_amd.mcmc import DIAG_FIELDS

    assert len(a) == len(b)
    for x, y in zip(a, b):
        for f in DIAG_FIELDS:
            assert np.asarray(x[f], np.float64).tobytes() == np.asarray(y[f], np.float64).tobytes(), f


def test_fit_diagnostics_equal_chainstats_of_the_chain_rows(lk, fitted):
    from transcriptioncycleinference_amd.mcmc import DIAG_FIELDS, THETA_INDEX, chain_theta, fit

    assert [d["cell_index"] for d in fitted.MCMCdiag] == [c + 1 for c in IDS]
    for d, ch, c in zip(fitted.MCMCdiag, fitted.MCMCchain, IDS):
        n = int(lk.cells.lengths[c])
        assert tuple(d) == DIAG_FIELDS and d["n_rows"] == 1501 == len(ch["v_chain"])
        th = chain_theta(ch, n, np.arange(1501))
        st = lk.chainstats(th, ch["s2chain"][499:])       # s2chain is not sliced by n_burn
        for stat, arr, s2 in (("mcerr", st.mcerr, st.s2_mcerr), ("tau", st.tau, st.s2_tau),
                              ("geweke_p", st.geweke_p, st.s2_geweke_p)):
            for name, col in THETA_INDEX.items():
                assert d[f"{stat}_{name}"] == arr[0, col], (stat, name)
            assert d[stat + "_dR"].tobytes() == arr[0, 7:].tobytes() and d[stat + "_s2"] == s2[0]
        assert d["ess_min"] == d["n_rows"] / st.tau[0].max()
        assert 0 < d["ess_min"] <= 2 * d["n_rows"]
    # a fit without diagnostics has none, and the same results
    plain = fit(lk, cells=IDS, **FIT)
    assert plain.MCMCdiag is None
    assert plain.MCMCchain[1]["dR_chain"].tobytes() == fitted.MCMCchain[1]["dR_chain"].tobytes()
    # a shard of the cells reproduces the full fit's entries bit for bit
    shard = fit(lk, cells=IDS[1:2], diagnostics=True, **FIT)
    _diag_equal(shard.MCMCdiag, fitted.MCMCdiag[1:2])


def _sharded_worker(rank, world, port, q):
    import os

    import torch.distributed as dist

    from transcriptioncycleinference_amd import Likelihood, testdata
    from transcriptioncycleinference_amd.parallel import fit_sharded, pack_diag

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cells = testdata().subset(IDS)
    with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as L:
        fr = fit_sharded(L, diagnostics=True, **FIT)
    if rank == 0:
        q.put((pack_diag(fr.MCMCdiag, int(cells.lengths.max())), fr.gather_bytes))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_fit_gathers_the_same_diagnostics():
    """fit_sharded over 2 ranks (gloo, both on this GPU) gathers the MCMCdiag of a one-process fit."""
    import socket

    import torch.multiprocessing as mp

    from transcriptioncycleinference_amd import Likelihood, testdata
    from transcriptioncycleinference_amd.mcmc import fit
    from transcriptioncycleinference_amd.parallel import fit_sharded, pack_diag, unpack_diag

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_sharded_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got, gbytes = q.get(timeout=240)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    cells = testdata().subset(IDS)
    with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as L:
        one = fit(L, diagnostics=True, **FIT)
        off = fit_sharded(L, **FIT)                     # no process group: one rank, diagnostics off
        on = fit_sharded(L, diagnostics=True, **FIT)
    want = pack_diag(one.MCMCdiag, int(cells.lengths.max()))
    assert got.tobytes() == want.tobytes()
    _diag_equal(unpack_diag(got), one.MCMCdiag)
    _diag_equal(on.MCMCdiag, one.MCMCdiag)
    assert off.MCMCdiag is None and on.gather_bytes == off.gather_bytes + want.nbytes == gbytes
