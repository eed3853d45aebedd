// tci_demczs_bounds.hip -- the kBounds instantiations of k_zs_propose and k_zs_decide (tci_demczs_kernels.h) and their
// launches, for tci_demczs_run_bounds: the per-coordinate bounds census and the oriented reflection (include/tci.h). A
// translation unit of its own, so that tci_demczs.hip's code object is the kernels of tci_demczs_run alone.
#include "tci_demczs_kernels.h"

namespace tci {

int launch_zs_propose_bounds(const KParams& kp, const int32_t* cell_id, const int64_t* keys, const double* pop,
                      const double* arch, const double* lower, const double* upper, const double* mu, const double* sig,
                      const double* jitter, int64_t n_sel, int64_t n_pop, int64_t M_g, int64_t M_cap, int64_t ld,
                      int64_t gen, bool jump, uint64_t seed, double gamma0, double CR, double p_snooker, double* trial,
                      double* pri, double* ljac, uint8_t* move, uint8_t* active, void* stream, const ZsBounds& bx) {
  const int rc = zs_sizes(n_sel, n_pop, M_g, M_cap, ld, gen);
  if (rc != TCI_OK) return rc;
  if (gen < 1 || !cell_id || !pop || !mu || !sig || !pri || !keys || !arch || !lower || !upper || !jitter || !trial || !ljac ||
      !move || !active)
    return TCI_EINVAL;
  if (!bx.n_left_t || !bx.n_refl_t || (bx.n_cross && (!bx.oob_lo || !bx.oob_hi)) ||
      (bx.reflect && (!bx.orient || !bx.orient_t)))
    return TCI_EINVAL;
  const int64_t B = n_sel * n_pop;
  const dim3 grid((unsigned)((B + kZsWaves - 1) / kZsWaves)), block(kZsThreads);
  hipLaunchKernelGGL((k_zs_propose<false, true, ZsBounds>), grid, block, 0, (hipStream_t)stream, kp.cells, cell_id, keys, pop, arch, lower,
                       upper, mu, sig, jitter, (uint32_t)n_pop, (uint32_t)M_g, M_cap, ld, B, gen, (int)jump, seed, gamma0, CR,
                       p_snooker, trial, pri, ljac, move, active, bx);
  return hipGetLastError() == hipSuccess ? TCI_OK : TCI_EHIP;
}

int launch_zs_decide_bounds(const KParams& kp, const int32_t* cell_id, const int64_t* keys, const double* sigma2_0,
                     const double* trial, const double* ss_t, const double* pri_t, const double* ljac, const uint8_t* move,
                     const uint8_t* active, int64_t n_sel, int64_t n_pop, int64_t M_cap, int64_t ld, int64_t gen,
                     uint64_t seed, bool updatesigma, int64_t keep_row, int64_t app_row, int64_t log_row, double* pop,
                     double* arch, double* ss, double* pri, double* s2, int32_t* n_acc, int32_t* n_oob, int32_t* n_null,
                     double* chain, double* s2chain, double* sschain, double* prichain, double* logr, uint8_t* acc_log,
                     uint8_t* oob_log, double* ljac_log, uint8_t* snk_log, void* stream, const ZsDecideBounds& bx) {
  const int rc = zs_sizes(n_sel, n_pop, 3, M_cap, ld, 0);
  if (rc != TCI_OK) return rc;
  if (gen < 1 || !cell_id || !sigma2_0 || !pop || !ss || !pri || !s2 || !n_acc || !n_oob || !n_null || !keys || !trial ||
      !ss_t || !pri_t || !ljac || !move || !active)
    return TCI_EINVAL;
  if (keep_row >= 0 && (!chain || !s2chain || !sschain || !prichain)) return TCI_EINVAL;
  if (app_row >= 0 && (!arch || app_row + n_pop > M_cap)) return TCI_EINVAL;
  if (!bx.n_left_t || !bx.n_refl_t || !bx.n_reflected || (bx.orient && !bx.orient_t)) return TCI_EINVAL;
  const int64_t B = n_sel * n_pop;
  const dim3 grid((unsigned)n_sel), block(kZsDecThreads);
  hipLaunchKernelGGL((k_zs_decide<false, true, ZsDecideBounds>), grid, block, 0, (hipStream_t)stream, kp.cells, cell_id, keys, sigma2_0, trial,
                       ss_t, pri_t, ljac, move, active, (int)n_pop, M_cap, ld, B, gen, seed, (int)updatesigma, keep_row,
                       app_row, log_row, pop, arch, ss, pri, s2, n_acc, n_oob, n_null, chain, s2chain, sschain, prichain, logr,
                       acc_log, oob_log, ljac_log, snk_log, bx);
  return hipGetLastError() == hipSuccess ? TCI_OK : TCI_EHIP;
}

}  // namespace tci
