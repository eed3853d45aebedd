"""Parallel tempering without a device: the ladder's inverse temperatures, the row layout of a tempered fit, the Python
wrappers' own argument checks, the restatement's pairing and exchange (tests/temper_oracle.py) on hand-worked cases and
MCMCtemper assembled from a synthetic DramResult."""
import ctypes as C
import math

import numpy as np
import pytest

import temper_oracle as TO


def test_temper_ladder_values():
    from transcriptioncycleinference_amd.mcmc import temper_ladder

    b = temper_ladder(8, 4)
    q = 1.0 / (1.0 + math.sqrt(2.0 / 8))     # = 2 / 3
    assert b.dtype == np.float64 and b[0] == 1.0
    np.testing.assert_allclose(b, [1.0, q, q * q, q ** 3], rtol=1e-15)
    np.testing.assert_allclose(q, 2.0 / 3.0, rtol=1e-15)
    np.testing.assert_array_equal(temper_ladder(19, 1), [1.0])
    np.testing.assert_array_equal(temper_ladder(19, 3, ratio=0.5), [1.0, 0.5, 0.25])
    assert np.all(np.diff(temper_ladder(207, 6)) < 0)
    # more dimensions, closer rungs: the energy distributions narrow as 1 / sqrt(P)
    assert temper_ladder(200, 2)[1] > temper_ladder(20, 2)[1]
    for bad in (dict(P=0, rungs=2), dict(P=5, rungs=0), dict(P=5, rungs=2, ratio=1.0), dict(P=5, rungs=2, ratio=0.0)):
        with pytest.raises(ValueError):
            temper_ladder(**bad)


def test_fit_row_layout_and_cold_rung_indices():
    from transcriptioncycleinference_amd.mcmc import REPLICATE_KEY_STRIDE, replicate_keys, temper_ladder, temper_layout

    lengths, M, R = [12, 17, 12], 2, 3
    K = len(lengths)
    lay = temper_layout(lengths, M, R)
    beta, ladder = lay["beta"], lay["ladder"]
    assert beta.shape == ladder.shape == (M * R * K,) and ladder.dtype == np.int32
    # the cold rungs come first, in the replicate-major order of an untempered fit
    assert np.all(beta[:M * K] == 1.0) and np.all(beta[M * K:] < 1.0)
    np.testing.assert_array_equal(ladder[:M * K], np.arange(M * K))
    for k, n in enumerate(lengths):
        want = temper_ladder(7 + n, R)
        for r in range(M):
            rungs = [(q * M + r) * K + k for q in range(R)]
            np.testing.assert_array_equal(beta[rungs], want)
            assert np.all(ladder[rungs] == r * K + k)
            assert TO.rungs(ladder)[r * K + k] == rungs          # ascending chain index = cold first
    one = temper_layout(lengths, M, R, betas=[1.0, 0.5, 0.2])
    np.testing.assert_array_equal(one["beta"], np.repeat([1.0, 0.5, 0.2], M * K))
    # a rung runs on the RNG stream of replicate q * M + r: distinct modulo 2^32
    keys = replicate_keys(np.arange(K) + 40, M * R)
    assert len(set(int(x) & 0xFFFFFFFF for x in keys)) == M * R * K
    assert keys[(2 * M + 1) * K + 1] == 41 + (2 * M + 1) * REPLICATE_KEY_STRIDE


def test_python_argument_errors():
    from transcriptioncycleinference_amd import _lib
    from transcriptioncycleinference_amd.build import build_library
    from transcriptioncycleinference_amd.mcmc import DramOptions, dram_run, fit, swap_event_rows

    build_library()
    lib = _lib.load()
    o = _lib.tci_temper_options(None, None, 7, 9, 3)
    assert lib.tci_temper_defaults(C.byref(o)) == _lib.TCI_OK
    assert (o.n_ladders, o.swap_every, o.flags) == (0, 1, 0) and not o.beta and not o.ladder
    assert lib.tci_temper_defaults(None) == _lib.TCI_EINVAL
    dopt, dout, tout = _lib.tci_dram_options(), _lib.tci_dram_outputs(), _lib.tci_temper_outputs()
    assert lib.tci_dram_run_tempered(None, C.byref(dopt), 2, None, None, None, None, None, None, None, None, 8,
                                     C.byref(dout), None, None, 0, None, None, C.byref(o),
                                     C.byref(tout)) == _lib.TCI_EINVAL
    for bad in (0, -1, 1.5, True, [0.9, 0.5], [1.0, 1.0], [1.0, 0.5, 0.7], [1.0, 0.0], [1.0, np.nan], []):
        with pytest.raises(ValueError, match="temper"):
            fit(object(), temper=bad)
    for bad in (-1, 0.5, True):
        with pytest.raises(ValueError, match="swap_every"):
            fit(object(), temper=2, swap_every=bad)
    with pytest.raises(ValueError, match="thin"):
        fit(object(), temper=2, replicates=2)             # MCMCrhat of the cold rungs needs the kept rows
    z = np.zeros((2, 8))
    for kw in (dict(ess=True, group=[0, 0]), dict(logpost=True)):
        with pytest.raises(ValueError, match="tempered"):
            dram_run(object(), [0, 0], z, z, z, z, z, z, 1.0, DramOptions(), beta=[1.0, 0.5], **kw)
    with pytest.raises(ValueError, match="swap_every"):
        dram_run(object(), [0, 0], z, z, z, z, z, z, 1.0, DramOptions(), ladder=[0, 0], swap_every=-1)
    # the rows the events follow: no window end, a window end on the last row, one past it
    assert len(swap_event_rows(15, 20, 1)) == 0
    np.testing.assert_array_equal(swap_event_rows(100, 20, 1), [20, 40, 60, 80])
    np.testing.assert_array_equal(swap_event_rows(101, 20, 1), [20, 40, 60, 80, 100])
    np.testing.assert_array_equal(swap_event_rows(101, 20, 2), [40, 80])
    np.testing.assert_array_equal(swap_event_rows(250, 0, 1), [100, 200])
    assert len(swap_event_rows(101, 20, 0)) == 0
    for a in ((15, 20, 1), (100, 20, 1), (101, 20, 1), (101, 20, 2), (250, 0, 1), (101, 20, 0), (1000, 7, 3)):
        np.testing.assert_array_equal(swap_event_rows(*a), TO.event_rows(*a))


def test_oracle_pairing_and_exchange_by_hand():
    ladder = np.array([0, 0, 1, 1, 1, -1, 2, 2, 2, 2])
    assert TO.rungs(ladder) == {0: [0, 1], 1: [2, 3, 4], 2: [6, 7, 8, 9]}
    # window 1: w / swap_every = 1 is odd, so the pairs (1, 2); a 2-rung ladder has none
    assert TO.pairs_tried(ladder, 20, 20, 1) == [(3, 4), (7, 8)]
    assert TO.pairs_tried(ladder, 40, 20, 1) == [(0, 1), (2, 3), (6, 7), (8, 9)]
    assert TO.pairs_tried(ladder, 40, 20, 2) == [(3, 4), (7, 8)]          # window 2 is event 1 of swap_every = 2
    assert TO.pairs_tried(ladder, 200, 0, 1) == [(0, 1), (2, 3), (6, 7), (8, 9)]
    # logr: equal deviances give 0; a hot rung at a lower ss makes the swap certain
    lr, bound = TO.logr(1.0, 0.5, 30.0, 1.0, 30.0, 2.0, 24)
    assert lr == 0.0 and bound > 0.0
    lr, _ = TO.logr(1.0, 0.5, 50.0, 1.0, 30.0, 2.0, 24)                  # sigma2 = 1 on both: dev_a - dev_b = 20
    assert lr == 0.25 * 20.0 and TO.accept(lr, 0.999999)
    lr, _ = TO.logr(1.0, 0.5, 30.0, 1.0, 50.0, 2.0, 24)
    assert lr == -5.0 and TO.accept(lr, 0.006) and not TO.accept(lr, 0.007)   # exp(-5) = 0.006738
    assert not TO.accept(np.nan, 1e-300) and not TO.accept(np.inf, 0.5) and not TO.accept(-np.inf, 0.5)
    # the uniform: inside (0, 1), a function of the whole key, the counter of Salmon et al.'s known-answer test
    assert TO.philox4x32_10([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    u = [TO.uniform_at(7, k, s) for k in (0, 1) for s in (20, 40)]
    assert len(set(u)) == 4 and all(0.0 < x < 1.0 for x in u)
    assert TO.uniform_at(7, 1, 20) != TO.uniform_at(7, 1, 20, purpose=2)
    # the exchange
    beta = np.array([1.0, 0.5])
    st = dict(theta=np.array([[1.0, 2.0], [3.0, 4.0]]), ss=np.array([10.0, 20.0]), prior=np.array([0.1, 0.2]),
              s2t=np.array([1.5, 4.0]))
    TO.exchange(st, 0, 1, beta, updatesigma=True)
    np.testing.assert_array_equal(st["theta"], [[3.0, 4.0], [1.0, 2.0]])
    np.testing.assert_array_equal(st["ss"], [20.0, 10.0])
    np.testing.assert_array_equal(st["prior"], [0.2, 0.1])
    np.testing.assert_array_equal(st["s2t"], [2.0, 3.0])       # physical 1.5 and 2.0 change places
    TO.exchange(st, 0, 1, beta, updatesigma=False)
    np.testing.assert_array_equal(st["s2t"], [2.0, 3.0])
    np.testing.assert_array_equal(st["ss"], [10.0, 20.0])


def test_mcmctemper_from_a_synthetic_result():
    from transcriptioncycleinference_amd.mcmc import TEMPER_FIELDS, DramResult, TemperResult, temper_entry, temper_layout

    K, M, R = 2, 2, 3
    n = K * M * R
    lay = temper_layout([12, 17], M, R, betas=[1.0, 0.6, 0.3])
    tried = np.zeros(n, np.int32)
    acc = np.zeros(n, np.int32)
    chain = lambda q, r, k: (q * M + r) * K + k  # noqa: E731
    tried[chain(0, 1, 1)], acc[chain(0, 1, 1)] = 10, 4     # cell 1, replicate 1, pair (0, 1)
    tried[chain(1, 1, 1)], acc[chain(1, 1, 1)] = 9, 9      # pair (1, 2)
    tried[chain(0, 0, 1)], acc[chain(0, 0, 1)] = 10, 0
    tr = TemperResult(lay["beta"], lay["ladder"], 2, tried, acc, np.zeros((0, n)), np.zeros((0, n), np.uint8),
                      np.zeros(0, np.int64), 19)
    rate = np.arange(n) / 100.0
    z = np.zeros((n, 24))
    res = DramResult(z, z, z, np.zeros(n), np.zeros(n), rate, np.zeros(n, np.int64), None, None, 0.0, temper=tr)
    e = temper_entry(res, 1, K, M, R, 42)
    assert tuple(e) == TEMPER_FIELDS
    np.testing.assert_array_equal(e["beta"], [1.0, 0.6, 0.3])
    np.testing.assert_array_equal(e["swap_tried"], [[10, 0], [10, 9]])
    assert e["swap_rate"][0, 0] == 0.0 and np.isnan(e["swap_rate"][0, 1])
    np.testing.assert_array_equal(e["swap_rate"][1], [0.4, 1.0])
    np.testing.assert_array_equal(e["accept_rate"], [[rate[chain(q, r, 1)] for q in range(R)] for r in range(M)])
    assert (e["swap_every"], e["n_events"], e["n_chains"], e["cell_index"]) == (2, 19, M * R, 42)
