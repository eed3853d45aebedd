"""The status code and the full tci_last_error text of the argument checks that the sampler's reductions and the
stand-alone chain entry points share: the kept-row window of every tci_dram_run_* reduction (thin, and the rows at or
past stats_from), which of two wrong reductions is reported (stats, cov, quantiles, densities, lp, group: the first
wins), and the npar range and n_rows minimum of every tci_chain* entry point. The Python wrappers reject most of
this input before the C ABI sees it, so the entry points are called through _lib directly. Every call fails before
any kernel is launched; the texts are the library's, letter for letter."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_CHAINS, N_STEPS = 2, 4
EINVAL, ERANGE = -1, -5


@pytest.fixture(scope="module")
def lk(cells):
    from transcriptioncycleinference_amd import Likelihood

    with Likelihood(cells.subset([int(np.argmin(cells.lengths))]), "P2P-MS2v5-LacZ-PP7v4", device=0) as L:
        yield L


def failure(lk, rc):
    return rc, lk._lib.tci_last_error(lk._h).decode()


# ---- the sampler's reductions: every output struct is zeroed (null arrays): no call gets as far as writing one

def dram(lk, entry, thin, stats_from, asks):
    """Call tci_dram_run_<entry> on two chains of four steps asking for the reductions named in `asks`."""
    from transcriptioncycleinference_amd import _lib
    from transcriptioncycleinference_amd.mcmc import DramOptions

    ld = 7 + int(lk.lengths[0])
    P = lambda a: _lib.ptr(a, _lib._dp)  # noqa: E731
    cid = np.zeros(N_CHAINS, np.int32)
    x, lo, hi, sig = np.zeros((N_CHAINS, ld)), np.full((N_CHAINS, ld), -1.0), np.ones((N_CHAINS, ld)), np.ones((N_CHAINS, ld))
    s20 = np.ones(N_CHAINS)
    o = DramOptions(n_steps=N_STEPS, burnintime=2, adaptint=2, stats_from=stats_from, thin=thin).to_c()
    out = _lib.tci_dram_outputs()
    args = (lk._h, C.byref(o), N_CHAINS, _lib.ptr(cid, _lib._i32p), P(x), P(lo), P(hi), P(x), P(sig), P(sig), P(s20), ld,
            C.byref(out))
    sout, cout = _lib.tci_chainstats_outputs(), _lib.tci_chaincov_outputs()
    qout, dout = _lib.tci_chainquant_outputs(), _lib.tci_chaindens_outputs()
    rout, eout, lout = _lib.tci_chainrhat_outputs(), _lib.tci_chainess_outputs(), _lib.tci_chainlp_outputs()
    red = _lib.tci_dram_reductions()
    if "stats" in asks:
        red.sout = C.pointer(sout)
    if "cov" in asks:
        red.cout = C.pointer(cout)
    if "quant" in asks:
        red.qout = C.pointer(qout)
    if "dens" in asks:
        red.dout = C.pointer(dout)
    grp = np.zeros(N_CHAINS, np.int32)
    group = (_lib.ptr(grp, _lib._i32p), 1, None, C.byref(rout))
    no_group = (None, 0, None, None)
    L = lk._lib
    if entry == "stats":
        rc = L.tci_dram_run_stats(*args, None, C.byref(sout))
    elif entry == "cov":
        rc = L.tci_dram_run_cov(*args, None, red.sout, None, C.byref(cout))
    elif entry == "reduced":
        rc = L.tci_dram_run_reduced(*args, C.byref(red))
    elif entry == "rhat":
        rc = L.tci_dram_run_rhat(*args, C.byref(red), *group)
    elif entry == "ess":
        rc = L.tci_dram_run_ess(*args, C.byref(red), *group, None, C.byref(eout))
    else:
        assert entry == "lp"
        rc = L.tci_dram_run_lp(*args, C.byref(red), *(group if "group" in asks else no_group), None, None, None,
                               C.byref(lout))
    return failure(lk, rc)


# (entry, what it asks for, who, the thin = 0 text, stats_from of a window one row short, that text)
NO_ROW = "no kept row at or past stats_from (n_rows < 1)"
ONE_ROW = "fewer than 2 kept rows at or past stats_from (n_rows < 2)"
WINDOWS = [
    ("stats", ("stats",), "tci_dram_run_stats", "the statistics need the kept rows (thin >= 1)", N_STEPS + 1, NO_ROW),
    ("cov", ("cov",), "tci_dram_run_cov", "the matrices need the kept rows (thin >= 1)", N_STEPS, ONE_ROW),
    ("reduced", ("quant",), "tci_dram_run_reduced", "the quantiles need the kept rows (thin >= 1)", N_STEPS + 1, NO_ROW),
    ("reduced", ("dens",), "tci_dram_run_reduced", "the densities need the kept rows (thin >= 1)", N_STEPS, ONE_ROW),
    ("lp", (), "tci_dram_run_lp", "the log-posterior trace needs the kept rows (thin >= 1)", N_STEPS + 1, NO_ROW),
    ("rhat", (), "tci_dram_run_rhat", "the group reduction needs the kept rows (thin >= 1)", N_STEPS, ONE_ROW),
    ("ess", (), "tci_dram_run_ess", "the group reduction needs the kept rows (thin >= 1)", N_STEPS, ONE_ROW),
]
WINDOW_IDS = ["stats", "cov", "quant", "dens", "lp", "rhat", "ess"]


@pytest.mark.parametrize("entry,asks,who,thin_text,short_from,short_text", WINDOWS, ids=WINDOW_IDS)
def test_reduction_without_kept_rows(lk, entry, asks, who, thin_text, short_from, short_text):
    assert dram(lk, entry, 0, 1, asks) == (EINVAL, f"{who}: {thin_text}")


@pytest.mark.parametrize("entry,asks,who,thin_text,short_from,short_text", WINDOWS, ids=WINDOW_IDS)
def test_reduction_window_one_row_short(lk, entry, asks, who, thin_text, short_from, short_text):
    assert dram(lk, entry, 1, short_from, asks) == (EINVAL, f"{who}: {short_text}")


# tci_dram_run_lp takes every reduction: with all of them wrong the first in the order stats, cov, quantiles,
# densities, lp, group is the one reported
ORDER = [
    (("stats", "cov", "quant", "dens", "group"), "tci_dram_run_stats: the statistics need the kept rows (thin >= 1)",
     "tci_dram_run_stats: no kept row at or past stats_from (n_rows < 1)"),
    (("cov", "quant", "dens", "group"), "tci_dram_run_cov: the matrices need the kept rows (thin >= 1)",
     "tci_dram_run_cov: fewer than 2 kept rows at or past stats_from (n_rows < 2)"),
    (("quant", "dens", "group"), "tci_dram_run_reduced: the quantiles need the kept rows (thin >= 1)",
     "tci_dram_run_reduced: no kept row at or past stats_from (n_rows < 1)"),
    (("dens", "group"), "tci_dram_run_reduced: the densities need the kept rows (thin >= 1)",
     "tci_dram_run_reduced: fewer than 2 kept rows at or past stats_from (n_rows < 2)"),
    (("group",), "tci_dram_run_lp: the log-posterior trace needs the kept rows (thin >= 1)",
     "tci_dram_run_lp: no kept row at or past stats_from (n_rows < 1)"),
]


@pytest.mark.parametrize("asks,thin_text,window_text", ORDER, ids=["stats", "cov", "quant", "dens", "lp"])
def test_first_wrong_reduction_wins(lk, asks, thin_text, window_text):
    assert dram(lk, "lp", 0, 1, asks) == (EINVAL, thin_text)
    assert dram(lk, "lp", 1, N_STEPS + 1, asks) == (EINVAL, window_text)


def test_group_reduction_is_checked_last(lk):
    """One row at or past stats_from: enough for the statistics, the quantiles and lp, one short for the group."""
    assert dram(lk, "lp", 1, N_STEPS, ("stats", "quant", "group")) == (
        EINVAL, "tci_dram_run_lp: fewer than 2 kept rows at or past stats_from (n_rows < 2)")
    assert dram(lk, "lp", 1, N_STEPS, ("stats", "cov", "quant", "group")) == (
        EINVAL, "tci_dram_run_cov: fewer than 2 kept rows at or past stats_from (n_rows < 2)")


# ---- the stand-alone entry points on a stored chain

def chain_call(lk, name, n_rows, npar=None, cell_id=(0, 0)):
    from transcriptioncycleinference_amd import _lib

    ld = 7 + int(lk.lengths[0])
    P = lambda a: _lib.ptr(a, _lib._dp)  # noqa: E731
    chain, s2 = np.zeros((max(n_rows, 1), N_CHAINS, ld)), np.ones((max(n_rows, 1), N_CHAINS))
    npar = None if npar is None else np.asarray(npar, np.int32)
    np_p = _lib.ptr(npar, _lib._i32p)
    out = getattr(_lib, f"tci_{name}_outputs")()
    fn, h = getattr(lk._lib, f"tci_{name}"), lk._h
    if name == "chaincov":
        rc = fn(h, None, P(chain), n_rows, N_CHAINS, ld, np_p, C.byref(out))
    elif name in ("chainrhat", "chainess"):
        rc = fn(h, None, P(chain), P(s2), n_rows, N_CHAINS, ld, np_p, None, 1, C.byref(out))
    elif name == "chainlp":
        cid, mu, sig = np.asarray(cell_id, np.int32), np.zeros((N_CHAINS, ld)), np.ones((N_CHAINS, ld))
        rc = fn(h, None, P(chain), P(s2), n_rows, N_CHAINS, ld, _lib.ptr(cid, _lib._i32p), P(mu), P(sig), C.byref(out))
    else:
        rc = fn(h, None, P(chain), P(s2), n_rows, N_CHAINS, ld, np_p, C.byref(out))
    return failure(lk, rc)


WITH_NPAR = ["chainstats", "chaincov", "chainquant", "chaindens", "chainrhat", "chainess"]
MIN_ROWS = {"chainstats": 1, "chaincov": 2, "chainquant": 1, "chaindens": 2, "chainrhat": 1, "chainess": 1, "chainlp": 1}


@pytest.mark.parametrize("name", WITH_NPAR)
def test_chain_npar_out_of_range(lk, name):
    ld = 7 + int(lk.lengths[0])
    for bad in (ld + 1, -1):
        assert chain_call(lk, name, N_STEPS, npar=[ld, bad]) == (ERANGE, f"tci_{name}: npar[1] outside [0, ld]")
    assert chain_call(lk, name, N_STEPS, npar=[-1, ld + 1]) == (ERANGE, f"tci_{name}: npar[0] outside [0, ld]")


def test_chainlp_cell_out_of_range(lk):
    """tci_chainlp takes cell ids where the others take npar (a chain's npar is its cell's 7 + N)."""
    for bad in (1, -1):
        assert chain_call(lk, "chainlp", N_STEPS, cell_id=(0, bad)) == (ERANGE, f"row 1: cell id {bad} out of range")


@pytest.mark.parametrize("name", WITH_NPAR + ["chainlp"])
def test_chain_too_few_rows(lk, name):
    m = MIN_ROWS[name]
    assert chain_call(lk, name, m - 1) == (EINVAL, f"tci_{name}: n_rows must be >= {m}")
