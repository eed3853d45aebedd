"""ctypes binding of the C ABI in ``include/tci.h`` (``libtci.so``, built in-tree for gfx950).

There is no fallback: if the library is missing the import of any compute entry point
raises :class:`TciLibraryMissing`. The product path never calls a CPU implementation.
"""
from __future__ import annotations

import ctypes as C
import os

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "libtci.so")

TCI_OK = 0
TCI_EINVAL = -1
TCI_EHIP = -2
TCI_ENOMEM = -3
TCI_EDIM = -4
TCI_ERANGE = -5
TCI_MAX_SEG = 4
TCI_MAX_POINTS = 2048
TCI_GRID_INTERP = 0
TCI_GRID_RAW = 1

_dp = C.POINTER(C.c_double)
_i64p = C.POINTER(C.c_int64)
_i32p = C.POINTER(C.c_int32)
_u8p = C.POINTER(C.c_uint8)


class TciLibraryMissing(ImportError):
    pass


class TciError(RuntimeError):
    """An error status returned through the C ABI (message from ``tci_last_error``)."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"[tci {code}] {msg}")
        self.code = code


class tci_cells(C.Structure):
    _fields_ = [("n_cells", C.c_int64), ("offsets", _i64p), ("t", _dp), ("ms2", _dp), ("pp7", _dp)]


class tci_construct(C.Structure):
    _fields_ = [("L0", C.c_double), ("n_seg", C.c_int32),
                ("ms2_start", _dp), ("ms2_end", _dp), ("ms2_loopn", _dp),
                ("pp7_start", _dp), ("pp7_end", _dp), ("pp7_loopn", _dp)]


class tci_info(C.Structure):
    _fields_ = [("device", C.c_int32), ("rows_per_lane", C.c_int32), ("n_cells", C.c_int64),
                ("max_points", C.c_int64), ("device_bytes", C.c_int64)]


class tci_dram_options(C.Structure):
    _fields_ = [("n_steps", C.c_int64), ("burnintime", C.c_int64), ("adaptint", C.c_int64), ("ntry", C.c_int32),
                ("updatesigma", C.c_int32), ("drscale", C.c_double), ("adascale", C.c_double),
                ("qcovadj", C.c_double), ("burnin_scale", C.c_double), ("stats_from", C.c_int64),
                ("thin", C.c_int64), ("seed", C.c_uint64), ("engine", C.c_int32), ("max_chunk", C.c_int32),
                ("chain_keys", C.POINTER(C.c_int64)), ("adapt_pmax", C.c_int64), ("kernel_times", C.c_int64)]


class tci_dram_outputs(C.Structure):
    _fields_ = [("mean", _dp), ("std", _dp), ("final_theta", _dp), ("sigma_mean", _dp), ("sigma_std", _dp),
                ("accept_rate", _dp), ("n_evals", _i64p), ("chain", _dp), ("s2chain", _dp), ("qcov_R", _dp),
                ("elapsed_ms", C.c_double), ("kernel_ms", C.c_double * 4), ("kernel_launches", C.c_int64 * 4)]


class tci_predict_options(C.Structure):
    _fields_ = [("grid_mode", C.c_int32), ("scratch_bytes", C.c_int64)]


class tci_chainstats_options(C.Structure):
    _fields_ = [("max_lag", C.c_int64)]


class tci_chainstats_outputs(C.Structure):
    _fields_ = [("mcerr", _dp), ("tau", _dp), ("geweke_z", _dp), ("geweke_p", _dp), ("tau_window", _i32p),
                ("s2_mcerr", _dp), ("s2_tau", _dp), ("s2_geweke_z", _dp), ("s2_geweke_p", _dp),
                ("s2_tau_window", _i32p), ("n_rows", C.c_int64), ("kernel_ms", C.c_double)]


class tci_chaincov_options(C.Structure):
    _fields_ = [("scratch_bytes", C.c_int64)]


class tci_chaincov_outputs(C.Structure):
    _fields_ = [("mean", _dp), ("cov", _dp), ("corr", _dp), ("n_rows", C.c_int64), ("kernel_ms", C.c_double)]


class tci_chainquant_options(C.Structure):
    _fields_ = [("nq", C.c_int32), ("probs", C.c_double * 16)]


class tci_chainquant_outputs(C.Structure):
    _fields_ = [("q", _dp), ("s2_q", _dp), ("n_rows", C.c_int64), ("kernel_ms", C.c_double)]


class tci_chaindens_options(C.Structure):
    _fields_ = [("n_grid", C.c_int32), ("n_bins", C.c_int32), ("bw_scale", C.c_double)]


class tci_chaindens_outputs(C.Structure):
    _fields_ = [("range", _dp), ("bw", _dp), ("dens", _dp), ("counts", _i32p), ("s2_range", _dp), ("s2_bw", _dp),
                ("s2_dens", _dp), ("s2_counts", _i32p), ("n_rows", C.c_int64), ("kernel_ms", C.c_double)]


class tci_chainlp_options(C.Structure):
    _fields_ = [("flags", C.c_int64)]


CHAINLP_TRACES = ("ss", "pri", "dev", "lp")
CHAINLP_SCALARS = ("ss_min", "ss_mean", "dev_mean", "dev_var", "lp_best", "ss_best", "s2_best", "s2_mean", "ss_hat",
                   "d_hat", "p_d", "p_v", "dic")


class tci_chainlp_outputs(C.Structure):
    _fields_ = ([(f, _dp) for f in CHAINLP_TRACES + CHAINLP_SCALARS]
                + [("best_row", _i64p), ("theta_best", _dp), ("theta_mean", _dp), ("n_rows", C.c_int64),
                   ("kernel_ms", C.c_double)])


class tci_dram_reductions(C.Structure):
    _fields_ = [("sopt", C.POINTER(tci_chainstats_options)), ("sout", C.POINTER(tci_chainstats_outputs)),
                ("copt", C.POINTER(tci_chaincov_options)), ("cout", C.POINTER(tci_chaincov_outputs)),
                ("qopt", C.POINTER(tci_chainquant_options)), ("qout", C.POINTER(tci_chainquant_outputs)),
                ("dopt", C.POINTER(tci_chaindens_options)), ("dout", C.POINTER(tci_chaindens_outputs))]


class tci_chainrhat_options(C.Structure):
    _fields_ = [("flags", C.c_int64)]


class tci_chainrhat_outputs(C.Structure):
    _fields_ = [("rhat", _dp), ("rhat_split", _dp), ("pooled_mean", _dp), ("pooled_std", _dp), ("s2_rhat", _dp),
                ("s2_rhat_split", _dp), ("s2_pooled_mean", _dp), ("s2_pooled_std", _dp), ("n_rows", C.c_int64),
                ("kernel_ms", C.c_double)]


class tci_chainess_options(C.Structure):
    _fields_ = [("max_lag", C.c_int64), ("flags", C.c_int64)]


class tci_chainess_outputs(C.Structure):
    _fields_ = [("ess", _dp), ("ess_split", _dp), ("tau", _dp), ("tau_split", _dp), ("mcse", _dp), ("window", _i32p),
                ("window_split", _i32p), ("s2_ess", _dp), ("s2_ess_split", _dp), ("s2_tau", _dp), ("s2_tau_split", _dp),
                ("s2_mcse", _dp), ("s2_window", _i32p), ("s2_window_split", _i32p), ("n_rows", C.c_int64),
                ("kernel_ms", C.c_double)]


class tci_chainrank_options(C.Structure):
    _fields_ = [("nq", C.c_int32), ("probs", C.c_double * 16), ("tail_lo", C.c_double), ("tail_hi", C.c_double),
                ("max_lag", C.c_int64), ("flags", C.c_int64)]


# per-group outputs of tci_chainrank, in the struct's order: doubles, then windows; each has an s2 twin
CHAINRANK_DOUBLES = ("q", "q_tail", "rhat_bulk", "rhat_folded", "rhat_rank", "ess_bulk", "tau_bulk", "ess_tail_lo",
                     "ess_tail_hi", "ess_tail")
CHAINRANK_WINDOWS = ("window_bulk", "window_tail_lo", "window_tail_hi")


class tci_chainrank_outputs(C.Structure):
    _fields_ = ([(f, _dp) for f in CHAINRANK_DOUBLES] + [(f, _i32p) for f in CHAINRANK_WINDOWS]
                + [("s2_" + f, _dp) for f in CHAINRANK_DOUBLES] + [("s2_" + f, _i32p) for f in CHAINRANK_WINDOWS]
                + [("z", _dp), ("z_folded", _dp), ("s2_z", _dp), ("s2_z_folded", _dp), ("n_rows", C.c_int64),
                   ("kernel_ms", C.c_double), ("rank_ms", C.c_double)])


class tci_temper_options(C.Structure):
    _fields_ = [("beta", _dp), ("ladder", _i32p), ("n_ladders", C.c_int64), ("swap_every", C.c_int64),
                ("flags", C.c_int64)]


class tci_temper_outputs(C.Structure):
    _fields_ = [("swap_tried", _i32p), ("swap_accepted", _i32p), ("swap_logr", _dp), ("swap_acc", _u8p),
                ("swap_log_rows", C.c_int64), ("n_events", C.c_int64)]


class tci_modesearch_options(C.Structure):
    _fields_ = [("n_gen", C.c_int64), ("F", C.c_double), ("CR", C.c_double), ("seed", C.c_uint64),
                ("keys", C.POINTER(C.c_int64)), ("flags", C.c_int64)]


class tci_modesearch_outputs(C.Structure):
    _fields_ = [("pop", _dp), ("f", _dp), ("ss", _dp), ("best", _i32p), ("theta_best", _dp), ("f_best", _dp),
                ("ss_best", _dp), ("pri_best", _dp), ("f_trace", _dp), ("n_accepted", _i32p), ("n_evals", C.c_int64),
                ("kernel_ms", C.c_double)]


class tci_demc_options(C.Structure):
    _fields_ = [("n_gen", C.c_int64), ("thin", C.c_int64), ("jump_every", C.c_int64), ("stats_from", C.c_int64),
                ("updatesigma", C.c_int64), ("CR", C.c_double), ("gamma0", C.c_double), ("seed", C.c_uint64),
                ("keys", C.POINTER(C.c_int64)), ("flags", C.c_int64)]


class tci_demc_outputs(C.Structure):
    _fields_ = [("chain", _dp), ("s2chain", _dp), ("sschain", _dp), ("prichain", _dp), ("pop", _dp), ("s2", _dp),
                ("ss", _dp), ("accept_rate", _dp), ("n_oob", _i32p), ("n_evals", _i64p), ("logr", _dp),
                ("accepted", _u8p), ("trial_oob", _u8p), ("log_rows", C.c_int64), ("n_keep", C.c_int64),
                ("kernel_ms", C.c_double)]


class tci_demczs_options(C.Structure):
    _fields_ = tci_demc_options._fields_ + [("append_every", C.c_int64), ("p_snooker", C.c_double)]


class tci_demczs_outputs(C.Structure):
    _fields_ = tci_demc_outputs._fields_ + [("n_null", _i32p), ("ljac", _dp), ("snooker", _u8p), ("archive", _dp),
                                            ("n_archive", C.c_int64)]


class tci_bounds_options(C.Structure):
    _fields_ = [("mode", C.c_int32), ("census", C.c_int32), ("flags", C.c_int64)]


class tci_bounds_outputs(C.Structure):
    _fields_ = [("n_cross", _i32p), ("oob_lo", _i32p), ("oob_hi", _i32p), ("n_left", _i32p), ("n_refl", _i32p),
                ("n_reflected", _i32p), ("orient", _u8p)]


TCI_BOUNDS_REJECT, TCI_BOUNDS_REFLECT = 0, 1


class tci_fitcheck_options(C.Structure):
    _fields_ = [("scratch_bytes", C.c_int64), ("n_levels", C.c_int32), ("levels", C.c_double * 8)]


class tci_fitcheck_outputs(C.Structure):
    _fields_ = [("lppd_i", _dp), ("p_waic_i", _dp), ("pit", _dp), ("resid", _dp), ("zbar", _dp), ("z2", _dp),
                ("n_obs", _i32p), ("lppd", _dp), ("p_waic", _dp), ("elpd_waic", _dp), ("chi2", _dp), ("coverage", _dp),
                ("dw", _dp), ("kernel_ms", C.c_double), ("forward_ms", C.c_double)]


class tci_loocheck_options(C.Structure):
    _fields_ = [("scratch_bytes", C.c_int64), ("n_groups", C.c_int64), ("khat_threshold", C.c_double),
                ("max_iter", C.c_int64), ("tol", C.c_double)]


LOOCHECK_POINTWISE = ("elpd_loo_i", "lppd_i", "p_loo_i", "khat_i")
LOOCHECK_SCALARS = ("elpd_loo", "p_loo", "lppd", "khat_max")


class tci_loocheck_outputs(C.Structure):
    _fields_ = ([(f, _dp) for f in LOOCHECK_POINTWISE] + [("n_obs", _i32p)] + [(f, _dp) for f in LOOCHECK_SCALARS]
                + [("n_khat_bad", _i32p), ("weight", _dp), ("elpd_stack", _dp), ("n_points", _i32p), ("n_iter", _i32p),
                   ("khat_threshold", C.c_double), ("kernel_ms", C.c_double), ("forward_ms", C.c_double)])


# (name, restype, argtypes) for every symbol declared in include/tci.h
SIGNATURES = [
    ("tci_construct_by_name", C.c_int, [C.c_char_p, C.POINTER(tci_construct)]),
    ("tci_create", C.c_int, [C.POINTER(tci_cells), C.POINTER(tci_construct), C.c_int, C.POINTER(C.c_void_p)]),
    ("tci_destroy", C.c_int, [C.c_void_p]),
    ("tci_last_error", C.c_char_p, [C.c_void_p]),
    ("tci_get_info", C.c_int, [C.c_void_p, C.POINTER(tci_info)]),
    ("tci_set_force_exact_scan", C.c_int, [C.c_void_p, C.c_int]),
    ("tci_ss_batch", C.c_int, [C.c_void_p, _dp, C.c_int64, _i32p, _u8p, C.c_int64, _dp]),
    ("tci_ss_batch_async", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.c_void_p, C.c_void_p]),
    ("tci_ssfun", C.c_int, [C.c_void_p, C.c_int32, _dp, C.c_int64, _dp]),
    ("tci_forward", C.c_int, [C.c_void_p, _dp, C.c_int64, _i32p, C.c_int64, C.c_int, _dp, _dp, C.c_int64]),
    ("tci_device_count", C.c_int, [C.POINTER(C.c_int)]),
    ("tci_cell_points", C.c_int, [C.c_void_p, C.c_int32, _i64p]),
    ("tci_cell_grid", C.c_int, [C.c_void_p, C.c_int32, _dp, C.c_int64, _i64p]),
    ("tci_dram_defaults", C.c_int, [C.POINTER(tci_dram_options)]),
    ("tci_dram_run", C.c_int, [C.c_void_p, C.POINTER(tci_dram_options), C.c_int64, _i32p, _dp, _dp, _dp, _dp, _dp,
                               _dp, _dp, C.c_int64, C.POINTER(tci_dram_outputs)]),
    ("tci_predict_defaults", C.c_int, [C.POINTER(tci_predict_options)]),
    ("tci_predict", C.c_int, [C.c_void_p, C.POINTER(tci_predict_options), _dp, C.c_int64, _i32p, C.c_int64, C.c_int64,
                              _dp, C.c_int32, _dp, _dp, C.c_int64]),
    ("tci_chainstats_defaults", C.c_int, [C.POINTER(tci_chainstats_options)]),
    ("tci_chainstats", C.c_int, [C.c_void_p, C.POINTER(tci_chainstats_options), _dp, _dp, C.c_int64, C.c_int64,
                                 C.c_int64, _i32p, C.POINTER(tci_chainstats_outputs)]),
    ("tci_dram_run_stats", C.c_int, [C.c_void_p, C.POINTER(tci_dram_options), C.c_int64, _i32p, _dp, _dp, _dp, _dp,
                                     _dp, _dp, _dp, C.c_int64, C.POINTER(tci_dram_outputs),
                                     C.POINTER(tci_chainstats_options), C.POINTER(tci_chainstats_outputs)]),
    ("tci_chaincov_defaults", C.c_int, [C.POINTER(tci_chaincov_options)]),
    ("tci_chaincov", C.c_int, [C.c_void_p, C.POINTER(tci_chaincov_options), _dp, C.c_int64, C.c_int64, C.c_int64,
                               _i32p, C.POINTER(tci_chaincov_outputs)]),
    ("tci_dram_run_cov", C.c_int, [C.c_void_p, C.POINTER(tci_dram_options), C.c_int64, _i32p, _dp, _dp, _dp, _dp,
                                   _dp, _dp, _dp, C.c_int64, C.POINTER(tci_dram_outputs),
                                   C.POINTER(tci_chainstats_options), C.POINTER(tci_chainstats_outputs),
                                   C.POINTER(tci_chaincov_options), C.POINTER(tci_chaincov_outputs)]),
    ("tci_chainquant_defaults", C.c_int, [C.POINTER(tci_chainquant_options)]),
    ("tci_chainquant", C.c_int, [C.c_void_p, C.POINTER(tci_chainquant_options), _dp, _dp, C.c_int64, C.c_int64,
                                 C.c_int64, _i32p, C.POINTER(tci_chainquant_outputs)]),
    ("tci_chaindens_defaults", C.c_int, [C.POINTER(tci_chaindens_options)]),
    ("tci_chaindens", C.c_int, [C.c_void_p, C.POINTER(tci_chaindens_options), _dp, _dp, C.c_int64, C.c_int64,
                                C.c_int64, _i32p, C.POINTER(tci_chaindens_outputs)]),
    ("tci_dram_run_reduced", C.c_int, [C.c_void_p, C.POINTER(tci_dram_options), C.c_int64, _i32p, _dp, _dp, _dp, _dp,
                                       _dp, _dp, _dp, C.c_int64, C.POINTER(tci_dram_outputs),
                                       C.POINTER(tci_dram_reductions)]),
    ("tci_chainrhat_defaults", C.c_int, [C.POINTER(tci_chainrhat_options)]),
    ("tci_chainrhat", C.c_int, [C.c_void_p, C.POINTER(tci_chainrhat_options), _dp, _dp, C.c_int64, C.c_int64,
                                C.c_int64, _i32p, _i32p, C.c_int64, C.POINTER(tci_chainrhat_outputs)]),
    ("tci_dram_run_rhat", C.c_int, [C.c_void_p, C.POINTER(tci_dram_options), C.c_int64, _i32p, _dp, _dp, _dp, _dp,
                                    _dp, _dp, _dp, C.c_int64, C.POINTER(tci_dram_outputs),
                                    C.POINTER(tci_dram_reductions), _i32p, C.c_int64,
                                    C.POINTER(tci_chainrhat_options), C.POINTER(tci_chainrhat_outputs)]),
    ("tci_chainess_defaults", C.c_int, [C.POINTER(tci_chainess_options)]),
    ("tci_chainess", C.c_int, [C.c_void_p, C.POINTER(tci_chainess_options), _dp, _dp, C.c_int64, C.c_int64,
                               C.c_int64, _i32p, _i32p, C.c_int64, C.POINTER(tci_chainess_outputs)]),
    ("tci_dram_run_ess", C.c_int, [C.c_void_p, C.POINTER(tci_dram_options), C.c_int64, _i32p, _dp, _dp, _dp, _dp,
                                   _dp, _dp, _dp, C.c_int64, C.POINTER(tci_dram_outputs),
                                   C.POINTER(tci_dram_reductions), _i32p, C.c_int64,
                                   C.POINTER(tci_chainrhat_options), C.POINTER(tci_chainrhat_outputs),
                                   C.POINTER(tci_chainess_options), C.POINTER(tci_chainess_outputs)]),
    ("tci_chainrank_defaults", C.c_int, [C.POINTER(tci_chainrank_options)]),
    ("tci_chainrank_lds_cap", C.c_int64, []),
    ("tci_chainrank", C.c_int, [C.c_void_p, C.POINTER(tci_chainrank_options), _dp, _dp, C.c_int64, C.c_int64,
                                C.c_int64, _i32p, _i32p, C.c_int64, C.POINTER(tci_chainrank_outputs)]),
    ("tci_dram_run_rank", C.c_int, [C.c_void_p, C.POINTER(tci_dram_options), C.c_int64, _i32p, _dp, _dp, _dp, _dp,
                                    _dp, _dp, _dp, C.c_int64, C.POINTER(tci_dram_outputs),
                                    C.POINTER(tci_dram_reductions), _i32p, C.c_int64,
                                    C.POINTER(tci_chainrhat_options), C.POINTER(tci_chainrhat_outputs),
                                    C.POINTER(tci_chainess_options), C.POINTER(tci_chainess_outputs),
                                    C.POINTER(tci_chainrank_options), C.POINTER(tci_chainrank_outputs)]),
    ("tci_fitcheck_defaults", C.c_int, [C.POINTER(tci_fitcheck_options)]),
    ("tci_fitcheck", C.c_int, [C.c_void_p, C.POINTER(tci_fitcheck_options), _dp, C.c_int64, _dp, _i32p, C.c_int64,
                               C.c_int64, C.c_int64, C.POINTER(tci_fitcheck_outputs)]),
    ("tci_loocheck_defaults", C.c_int, [C.POINTER(tci_loocheck_options)]),
    ("tci_loocheck", C.c_int, [C.c_void_p, C.POINTER(tci_loocheck_options), _dp, C.c_int64, _dp, _i32p, _i32p, C.c_int64,
                               C.c_int64, C.c_int64, C.POINTER(tci_loocheck_outputs)]),
    ("tci_chainlp_defaults", C.c_int, [C.POINTER(tci_chainlp_options)]),
    ("tci_chainlp", C.c_int, [C.c_void_p, C.POINTER(tci_chainlp_options), _dp, _dp, C.c_int64, C.c_int64, C.c_int64,
                              _i32p, _dp, _dp, C.POINTER(tci_chainlp_outputs)]),
    ("tci_dram_run_lp", C.c_int, [C.c_void_p, C.POINTER(tci_dram_options), C.c_int64, _i32p, _dp, _dp, _dp, _dp,
                                  _dp, _dp, _dp, C.c_int64, C.POINTER(tci_dram_outputs),
                                  C.POINTER(tci_dram_reductions), _i32p, C.c_int64,
                                  C.POINTER(tci_chainrhat_options), C.POINTER(tci_chainrhat_outputs),
                                  C.POINTER(tci_chainess_options), C.POINTER(tci_chainess_outputs),
                                  C.POINTER(tci_chainlp_options), C.POINTER(tci_chainlp_outputs)]),
    ("tci_temper_defaults", C.c_int, [C.POINTER(tci_temper_options)]),
    ("tci_dram_run_tempered", C.c_int, [C.c_void_p, C.POINTER(tci_dram_options), C.c_int64, _i32p, _dp, _dp, _dp, _dp,
                                        _dp, _dp, _dp, C.c_int64, C.POINTER(tci_dram_outputs),
                                        C.POINTER(tci_dram_reductions), _i32p, C.c_int64,
                                        C.POINTER(tci_chainrhat_options), C.POINTER(tci_chainrhat_outputs),
                                        C.POINTER(tci_temper_options), C.POINTER(tci_temper_outputs)]),
    ("tci_modesearch_defaults", C.c_int, [C.POINTER(tci_modesearch_options)]),
    ("tci_modesearch", C.c_int, [C.c_void_p, C.POINTER(tci_modesearch_options), _dp, C.c_int64, _i32p, C.c_int64,
                                 C.c_int64, _dp, _dp, _dp, _dp, _dp, C.POINTER(tci_modesearch_outputs)]),
    ("tci_demc_defaults", C.c_int, [C.POINTER(tci_demc_options)]),
    ("tci_demc_run", C.c_int, [C.c_void_p, C.POINTER(tci_demc_options), _dp, C.c_int64, _i32p, C.c_int64, C.c_int64, _dp,
                               _dp, _dp, _dp, _dp, _dp, C.POINTER(tci_demc_outputs),
                               C.POINTER(tci_chainrhat_options), C.POINTER(tci_chainrhat_outputs),
                               C.POINTER(tci_chainess_options), C.POINTER(tci_chainess_outputs)]),
    ("tci_demc_run_rank", C.c_int, [C.c_void_p, C.POINTER(tci_demc_options), _dp, C.c_int64, _i32p, C.c_int64, C.c_int64,
                                    _dp, _dp, _dp, _dp, _dp, _dp, C.POINTER(tci_demc_outputs),
                                    C.POINTER(tci_chainrhat_options), C.POINTER(tci_chainrhat_outputs),
                                    C.POINTER(tci_chainess_options), C.POINTER(tci_chainess_outputs),
                                    C.POINTER(tci_chainrank_options), C.POINTER(tci_chainrank_outputs)]),
    ("tci_demczs_defaults", C.c_int, [C.POINTER(tci_demczs_options)]),
    ("tci_demczs_run", C.c_int, [C.c_void_p, C.POINTER(tci_demczs_options), _dp, _dp, C.c_int64, _i32p, C.c_int64,
                                 C.c_int64, C.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, C.POINTER(tci_demczs_outputs),
                                 C.POINTER(tci_chainrhat_options), C.POINTER(tci_chainrhat_outputs),
                                 C.POINTER(tci_chainess_options), C.POINTER(tci_chainess_outputs)]),
    ("tci_demczs_run_rank", C.c_int, [C.c_void_p, C.POINTER(tci_demczs_options), _dp, _dp, C.c_int64, _i32p, C.c_int64,
                                      C.c_int64, C.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, C.POINTER(tci_demczs_outputs),
                                      C.POINTER(tci_chainrhat_options), C.POINTER(tci_chainrhat_outputs),
                                      C.POINTER(tci_chainess_options), C.POINTER(tci_chainess_outputs),
                                      C.POINTER(tci_chainrank_options), C.POINTER(tci_chainrank_outputs)]),
    ("tci_bounds_defaults", C.c_int, [C.POINTER(tci_bounds_options)]),
    ("tci_demczs_run_bounds", C.c_int, [C.c_void_p, C.POINTER(tci_demczs_options), _dp, _dp, C.c_int64, _i32p, C.c_int64,
                                        C.c_int64, C.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, C.POINTER(tci_demczs_outputs),
                                        C.POINTER(tci_chainrhat_options), C.POINTER(tci_chainrhat_outputs),
                                        C.POINTER(tci_chainess_options), C.POINTER(tci_chainess_outputs),
                                        C.POINTER(tci_chainrank_options), C.POINTER(tci_chainrank_outputs),
                                        C.POINTER(tci_bounds_options), C.POINTER(tci_bounds_outputs)]),
    ("tci_version", C.c_char_p, []),
]

_lib = None


def load(path: str | None = None):
    """Load ``libtci.so`` (raises :class:`TciLibraryMissing` when it has not been built)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise TciLibraryMissing(
            f"{p} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()')")
    lib = C.CDLL(p)
    for name, res, args in SIGNATURES:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def ptr(a, typ):
    return None if a is None else a.ctypes.data_as(typ)
