// tci_demczs.hip -- DE-MC(zs) (ter Braak & Vrugt 2008): a few chains per cell whose difference vectors come from an
// archive Z of past states, with snooker moves; a third sampler beside DRAM and DE-MC (tci_demc.hip). The definition is
// in include/tci.h (tci_demczs_run).
//
// The chains lie as [n_sel][n_pop][ld]; row b = k * n_pop + i is chain i of selected cell k, and ss, pri, s2, the
// counters, the trial buffer and its ss, pri, ljac, move and active vectors are laid out as the rows are: the archive
// does not depend on the other chains' current states, so every chain moves in every generation and a generation is
// three launches on one stream, one likelihood launch where DE-MC has two:
//   k_zs_propose   one wavefront per chain. Every lane repeats the two index calls (a, c, e, jrand; the move type and
//                  gamma_s), so the move type is wave-uniform and the two moves are two branches with no divergence.
//                  Parallel move: k_demc_propose's two passes with x_r1 = Z[a] and x_r2 = Z[c] (one Philox call per
//                  coordinate in pass 1, the crossing flags in a 64-bit mask, the jitter uniform parked in the trial
//                  entry; pass 2 runs no generator). Snooker move: no coordinate generator at all; pass 1 sums D and A,
//                  pass 2 forms the trial entries, tests the bounds and sums D'. The three sums combine their 64 lane
//                  partials by the xor butterfly, six dependent steps where prior_sum64 takes 64. A row that is out of
//                  bounds or null gets active = 0 and no prior; any other row's prior is summed in tci_chainlp's order
//                  (tci_prior.h), because prichain must keep equalling tci_chainlp's bits.
//   (the batched likelihood kernel, tci_kernels.hip, on the trial buffer under the active mask: launched by the host)
//   k_zs_decide    one workgroup per cell, shaped as k_demc_decide. A thread per chain adds ljac into logr, decides,
//                  draws the chain's sigma2 and stores its values, with the decision in LDS; after the barrier the waves
//                  stride over the chains and copy every accepted trial over its parent; after a second barrier, on an
//                  append generation the n_pop current rows go to archive rows M_g .. M_g + n_pop - 1 (rows no proposal
//                  of this generation read, and the next generation's launch is ordered after this one on the stream),
//                  and on a kept generation the kept rows are stored.
// Either kernel has a second template flag, kBounds, for tci_demczs_run_bounds (the per-coordinate bounds census and the
// oriented reflection; include/tci.h): the census and the reflection ride in pass 2 of the move they belong to, the
// per-proposal counts n_left and n_refl go through two [B] vectors to k_zs_decide, which logs them, counts the evaluated
// reflected proposals and copies the trial's orientation row with an accepted parallel trial. Row b's counters and
// orientation bytes are touched by row b's wavefront alone (lane l owns j = l, l + 64, ..), with plain vector loads and
// stores; the launches are ordered on the stream. The kernels are templates in tci_demczs_kernels.h; this file
// instantiates and launches the ones without the flag, which are what they were before it existed and are the only
// kernels of this file's code object, and tci_demczs_bounds.hip the ones with it.
// The archive lies as [n_sel][M_cap][ld], M_cap the final row count; generation g reads its first M_g rows.
// Bits: a chain's trial depends on the cell's archive rows below M_g, the chain's state, bounds, jitter, key, seed,
// generation and chain index alone. Every loop is bounded by an integer count.
#include "tci_demczs_kernels.h"

namespace tci {

int launch_zs_propose(const KParams& kp, const int32_t* cell_id, const int64_t* keys, const double* pop,
                      const double* arch, const double* lower, const double* upper, const double* mu, const double* sig,
                      const double* jitter, int64_t n_sel, int64_t n_pop, int64_t M_g, int64_t M_cap, int64_t ld,
                      int64_t gen, bool jump, uint64_t seed, double gamma0, double CR, double p_snooker, double* trial,
                      double* pri, double* ljac, uint8_t* move, uint8_t* active, void* stream, const ZsBounds* bx) {
  if (bx && gen > 0)  // the kBounds instantiation: a translation unit of its own
    return launch_zs_propose_bounds(kp, cell_id, keys, pop, arch, lower, upper, mu, sig, jitter, n_sel, n_pop, M_g, M_cap, ld,
                                    gen, jump, seed, gamma0, CR, p_snooker, trial, pri, ljac, move, active, stream, *bx);
  const int rc = zs_sizes(n_sel, n_pop, M_g, M_cap, ld, gen);
  if (rc != TCI_OK) return rc;
  if (!cell_id || !pop || !mu || !sig || !pri) return TCI_EINVAL;
  if (gen > 0 && (!keys || !arch || !lower || !upper || !jitter || !trial || !ljac || !move || !active)) return TCI_EINVAL;
  const int64_t B = n_sel * n_pop;
  const dim3 grid((unsigned)((B + kZsWaves - 1) / kZsWaves)), block(kZsThreads);
  if (gen == 0)
    hipLaunchKernelGGL((k_zs_propose<true, false>), grid, block, 0, (hipStream_t)stream, kp.cells, cell_id, keys, pop, arch, lower,
                       upper, mu, sig, jitter, (uint32_t)n_pop, (uint32_t)M_g, M_cap, ld, B, gen, (int)jump, seed, gamma0, CR,
                       p_snooker, trial, pri, ljac, move, active);
  else
    hipLaunchKernelGGL((k_zs_propose<false, false>), grid, block, 0, (hipStream_t)stream, kp.cells, cell_id, keys, pop, arch, lower,
                       upper, mu, sig, jitter, (uint32_t)n_pop, (uint32_t)M_g, M_cap, ld, B, gen, (int)jump, seed, gamma0, CR,
                       p_snooker, trial, pri, ljac, move, active);
  return hipGetLastError() == hipSuccess ? TCI_OK : TCI_EHIP;
}

int launch_zs_decide(const KParams& kp, const int32_t* cell_id, const int64_t* keys, const double* sigma2_0,
                     const double* trial, const double* ss_t, const double* pri_t, const double* ljac, const uint8_t* move,
                     const uint8_t* active, int64_t n_sel, int64_t n_pop, int64_t M_cap, int64_t ld, int64_t gen,
                     uint64_t seed, bool updatesigma, int64_t keep_row, int64_t app_row, int64_t log_row, double* pop,
                     double* arch, double* ss, double* pri, double* s2, int32_t* n_acc, int32_t* n_oob, int32_t* n_null,
                     double* chain, double* s2chain, double* sschain, double* prichain, double* logr, uint8_t* acc_log,
                     uint8_t* oob_log, double* ljac_log, uint8_t* snk_log, void* stream, const ZsDecideBounds* bx) {
  if (bx && gen > 0)
    return launch_zs_decide_bounds(kp, cell_id, keys, sigma2_0, trial, ss_t, pri_t, ljac, move, active, n_sel, n_pop, M_cap, ld,
                                   gen, seed, updatesigma, keep_row, app_row, log_row, pop, arch, ss, pri, s2, n_acc, n_oob,
                                   n_null, chain, s2chain, sschain, prichain, logr, acc_log, oob_log, ljac_log, snk_log, stream,
                                   *bx);
  const int rc = zs_sizes(n_sel, n_pop, 3, M_cap, ld, 0);
  if (rc != TCI_OK) return rc;
  if (!cell_id || !sigma2_0 || !pop || !ss || !pri || !s2 || !n_acc || !n_oob || !n_null) return TCI_EINVAL;
  if (gen > 0 && (!keys || !trial || !ss_t || !pri_t || !ljac || !move || !active)) return TCI_EINVAL;
  if (keep_row >= 0 && (!chain || !s2chain || !sschain || !prichain)) return TCI_EINVAL;
  if (app_row >= 0 && (!arch || app_row + n_pop > M_cap)) return TCI_EINVAL;
  const int64_t B = n_sel * n_pop;
  const dim3 grid((unsigned)n_sel), block(kZsDecThreads);
  if (gen == 0)
    hipLaunchKernelGGL((k_zs_decide<true, false>), grid, block, 0, (hipStream_t)stream, kp.cells, cell_id, keys, sigma2_0, trial,
                       ss_t, pri_t, ljac, move, active, (int)n_pop, M_cap, ld, B, gen, seed, (int)updatesigma, keep_row,
                       app_row, log_row, pop, arch, ss, pri, s2, n_acc, n_oob, n_null, chain, s2chain, sschain, prichain, logr,
                       acc_log, oob_log, ljac_log, snk_log);
  else
    hipLaunchKernelGGL((k_zs_decide<false, false>), grid, block, 0, (hipStream_t)stream, kp.cells, cell_id, keys, sigma2_0, trial,
                       ss_t, pri_t, ljac, move, active, (int)n_pop, M_cap, ld, B, gen, seed, (int)updatesigma, keep_row,
                       app_row, log_row, pop, arch, ss, pri, s2, n_acc, n_oob, n_null, chain, s2chain, sschain, prichain, logr,
                       acc_log, oob_log, ljac_log, snk_log);
  return hipGetLastError() == hipSuccess ? TCI_OK : TCI_EHIP;
}

}  // namespace tci
