"""fit(..., replicates=M, rank=...) and fit(..., demc=..., rank=...): MCMCrank against Likelihood.chainrank bit for bit,
the same fit without it byte for byte, the host route (with logpost or temper) against the device route, the .mat
round trip, and rank without replicates raising as ess does."""
import numpy as np
import pytest

IDS = [3, 41]


@pytest.fixture(scope="module")
def lk(cells):
    from transcriptioncycleinference_amd import Likelihood

    with Likelihood(cells, "P2P-MS2v5-LacZ-PP7v4", device=0) as lk:
        yield lk


def flat(x):
    if isinstance(x, dict):
        return b"".join(flat(x[k]) for k in sorted(x))
    return np.ascontiguousarray(x).tobytes()


def test_rank_needs_groups_without_a_gpu():
    from transcriptioncycleinference_amd import mcmc

    assert "MCMCrank" in mcmc.FitResult.__dataclass_fields__ and mcmc.RANK_FIELDS[:4] == ("q", "q_tail", "probs", "tail")

    class NoCells:          # fit refuses before it looks at the cells
        cells = None

    for kw in (dict(rank=True), dict(rank=True, replicates=1), dict(rank=dict(probs=(0.5,)), rhat=False, replicates=2)):
        with pytest.raises(ValueError, match="MCMCrank"):
            mcmc.fit(NoCells(), thin=1, **kw)
    with pytest.raises(ValueError, match="rank"):
        mcmc.fit(NoCells(), thin=1, replicates=2, rank=dict(quantiles=(0.5,)))
    with pytest.raises(ValueError):                           # rank needs group, as ess does
        mcmc.dram_run(None, np.zeros(1, np.int32), *(np.ones((1, 8)),) * 6, 1.0, mcmc.DramOptions(), rank=True)


@pytest.mark.gpu
def test_fit_replicates_with_rank(lk, tmp_path):
    import scipy.io as sio

    from transcriptioncycleinference_amd.mcmc import (RANK_FIELDS, RANK_VECTORS, DramOptions, dram_run, fit, plan_fit,
                                                      replicate_keys, save_results)

    kw = dict(n_steps=500, n_burn=150, thin=1, seed=11, cells=IDS, replicates=3)
    base = fit(lk, **kw)
    ranked = fit(lk, rank=dict(probs=(0.1, 0.5, 0.9), tail=(0.1, 0.9)), max_lag=40, **kw)
    assert base.MCMCrank is None and len(ranked.MCMCrank) == 2
    for name in ("MCMCresults", "MCMCchain", "MCMCplot", "MCMCrhat"):   # the same fit without rank, byte for byte
        for a, b in zip(getattr(base, name), getattr(ranked, name)):
            assert flat(a) == flat(b), name
    # the entries are Likelihood.chainrank of the replicates' kept rows, trimmed to P with s2 last
    p = plan_fit(lk.cells, IDS, 11, replicates=3)
    o = DramOptions(n_steps=500, burnintime=150, stats_from=150, thin=1, seed=11 * 1000003 + 20201028)
    res = dram_run(lk, np.tile(np.array(IDS, np.int32), 3), p.x0, p.lower, p.upper, p.prior_mu, p.prior_sig, p.qcov_diag,
                   1.0, o, chain_keys=replicate_keys(np.array(IDS, np.int64), 3))
    npar = (7 + lk.cells.lengths[np.tile(IDS, 3)]).astype(np.int32)
    want = lk.chainrank(res.chain[149:], res.s2chain[149:], npar, np.tile(np.arange(2, dtype=np.int32), 3),
                        probs=(0.1, 0.5, 0.9), tail=(0.1, 0.9), max_lag=40)
    for k, c in enumerate(IDS):
        e, P = ranked.MCMCrank[k], 7 + int(lk.cells.lengths[c])
        assert tuple(e) == RANK_FIELDS and e["n_rows"] == 351 and e["n_chains"] == 3 and e["cell_index"] == c + 1
        assert e["max_lag"] == 40 and e["q"].shape == (3, P + 1) and e["q_tail"].shape == (2, P + 1)
        for f in RANK_VECTORS:
            assert e[f].shape == (P + 1,)
            assert e[f].tobytes() == np.append(getattr(want, f)[k, :P], getattr(want, "s2_" + f)[k]).tobytes(), f
        for f in ("q", "q_tail"):
            assert e[f].tobytes() == np.concatenate([getattr(want, f)[k, :, :P], getattr(want, "s2_" + f)[k][:, None]],
                                                    axis=1).tobytes(), f
        assert e["window_bulk"].dtype == np.int32 and e["rhat_rank_max"] == np.nanmax(e["rhat_rank"])
        assert e["ess_bulk_min"] == np.nanmin(e["ess_bulk"]) and e["ess_tail_min"] == np.nanmin(e["ess_tail"])
        assert list(e["probs"]) == [0.1, 0.5, 0.9] and list(e["tail"]) == [0.1, 0.9]
    # with logpost no entry point takes rank: the kept rows go through tci_chainrank, the same bits
    hosted = fit(lk, rank=dict(probs=(0.1, 0.5, 0.9), tail=(0.1, 0.9)), max_lag=40, logpost=True, **kw)
    for a, b in zip(ranked.MCMCrank, hosted.MCMCrank):
        assert flat(a) == flat(b)
    # the .mat round trip, beside MCMCrhat
    path = save_results(ranked, str(tmp_path), date="01-Jan-2021")[0]
    d = sio.loadmat(path, struct_as_record=False, squeeze_me=True)
    assert list(d["MCMCrank"][0]._fieldnames) == list(RANK_FIELDS) and "MCMCrhat" in d
    for k in range(2):
        for f in RANK_VECTORS + ("q", "q_tail"):
            np.testing.assert_array_equal(np.asarray(getattr(d["MCMCrank"][k], f), np.float64),
                                          ranked.MCMCrank[k][f].astype(np.float64), err_msg=f)
    assert "MCMCrank" not in sio.loadmat(save_results(base, str(tmp_path), date="02-Jan-2021")[0])
    with pytest.raises(ValueError):
        fit(lk, rank=True, **{**kw, "replicates": 1})


@pytest.mark.gpu
def test_fit_tempered_and_demc_with_rank(lk):
    from transcriptioncycleinference_amd.mcmc import DEMC_FIELDS, RANK_FIELDS, demc, fit, rank_entry

    fr = fit(lk, n_steps=400, n_burn=100, thin=1, seed=3, cells=IDS, replicates=2, temper=2, rank=True)
    assert len(fr.MCMCrank) == 2 and fr.MCMCrank[0]["n_chains"] == 2 and fr.MCMCrank[0]["n_rows"] == 301
    assert np.all(np.isfinite(fr.MCMCrank[0]["rhat_rank"]))
    kw = dict(n_burn=4, thin=2, seed=3, cells=IDS)
    plain = fit(lk, demc=dict(n_pop=8, n_gen=12), **kw)
    ranked = fit(lk, demc=dict(n_pop=8, n_gen=12), rank=True, **kw)
    res, _ = demc(lk, n_pop=8, n_gen=12, rank=True, **kw)
    for k, c in enumerate(IDS):
        e = ranked.MCMCdemc[k]
        assert tuple(plain.MCMCdemc[k]) == DEMC_FIELDS and flat(plain.MCMCdemc[k]) == flat({f: e[f] for f in DEMC_FIELDS})
        want = rank_entry(res.rank, k, int(lk.cells.lengths[c]), c + 1, 8)
        extra = [f for f in RANK_FIELDS if f not in DEMC_FIELDS]
        assert tuple(e) == DEMC_FIELDS + tuple(extra) and flat({f: e[f] for f in extra}) == flat({f: want[f] for f in extra})
    for name in ("MCMCresults", "MCMCchain"):
        for a, b in zip(getattr(plain, name), getattr(ranked, name)):
            assert flat(a) == flat(b), name
