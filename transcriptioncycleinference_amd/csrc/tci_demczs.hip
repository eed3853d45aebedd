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
// The archive lies as [n_sel][M_cap][ld], M_cap the final row count; generation g reads its first M_g rows.
// Bits: a chain's trial depends on the cell's archive rows below M_g, the chain's state, bounds, jitter, key, seed,
// generation and chain index alone. Every loop is bounded by an integer count.
#include <hip/hip_runtime.h>
#include <math.h>

#include "tci_fp.h"
#include "tci_gamma.h"
#include "tci_internal.h"
#include "tci_prior.h"
#include "tci_rng.h"

namespace tci {

namespace {

constexpr int kZsThreads = 256;
constexpr int kZsWaves = kZsThreads / 64;
constexpr int kZsDecThreads = 1024;  // k_zs_decide: one workgroup per cell
constexpr int kZsDecWaves = kZsDecThreads / 64;
constexpr int kZsMaxPop = 4096;
// 9-12 are the DE-MC sampler's (tci_demc.hip)
constexpr uint32_t kPurposeIndex = 13, kPurposeCoord = 14, kPurposeAccept = 15, kPurposeSigma = 16;
// the coordinate counter i * 4096 + j, as k_demc_propose's
static_assert(7 + TCI_MAX_POINTS <= 4096, "the coordinate counter of k_zs_propose");
static_assert((7 + TCI_MAX_POINTS + 63) / 64 <= 64, "the crossing mask of k_zs_propose");

// m(w, n) of include/tci.h: a word scaled to [0, n)
__device__ __forceinline__ uint32_t zs_scale(uint32_t w, uint32_t n) { return (uint32_t)(((uint64_t)w * n) >> 32); }

// The 64 lane partials by the xor butterfly: addition commutes bitwise, so every lane holds the same value.
__device__ __forceinline__ double zs_sum64(double p) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) p = p + __shfl_xor(p, d, 64);
  return p;
}

// kInit: the prior of every chain's start (nothing but pop, mu and sig is read). Else: the trial of every chain in
// generation gen, from the first M_g rows of its cell's archive. B = n_sel * n_pop rows either way.
template <bool kInit>
__global__ __launch_bounds__(kZsThreads) void k_zs_propose(
    const CellMeta* __restrict__ cells, const int32_t* __restrict__ cell_id, const int64_t* __restrict__ keys,
    const double* __restrict__ pop, const double* __restrict__ arch, const double* __restrict__ lower,
    const double* __restrict__ upper, const double* __restrict__ mu, const double* __restrict__ sig,
    const double* __restrict__ jitter, uint32_t n_pop, uint32_t M_g, int64_t M_cap, int64_t ld, int64_t B, int64_t gen,
    int jump, uint64_t seed, double gamma0, double CR, double p_snooker, double* trial, double* __restrict__ pri,
    double* __restrict__ ljac, uint8_t* __restrict__ move, uint8_t* __restrict__ active) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.x * kZsWaves + wave;
  if (b >= B) return;                              // the whole wavefront
  const uint32_t k = (uint32_t)b / n_pop, i = (uint32_t)b % n_pop;  // B < 2^31 (the host checked): 32-bit divisions
  const int P = 7 + cells[cell_id[k]].n;           // <= ld (the host checked)
  if (kInit) {
    const double tot = prior_sum64(pop + b * ld, mu + (int64_t)k * ld, sig + (int64_t)k * ld, P, lane);
    if (lane == 0) pri[b] = tot;
    return;
  }
  const int64_t key = keys[k];
  const uint4 w = rng(seed, key, gen, kPurposeIndex, i);
  const uint4 q = rng(seed, key, gen, kPurposeIndex, (uint32_t)kZsMaxPop + i);
  const uint32_t a = zs_scale(w.x, M_g);           // M_g >= 3 (the host checked m0)
  uint32_t c = zs_scale(w.y, M_g - 1);
  c += c >= a;
  const bool snk = u01(q.x, q.y) < p_snooker;      // every lane alike: wave-uniform
  const double* Z = arch + (int64_t)k * M_cap * ld;
  const double* xi = pop + b * ld;
  const double* lo = lower + (int64_t)k * ld;
  const double* up = upper + (int64_t)k * ld;
  double* tr = trial + b * ld;
  bool oob = false;
  double lj = 0.0;
  if (snk) {
    const uint32_t mn = a < c ? a : c, mx = a < c ? c : a;
    uint32_t e = zs_scale(w.w, M_g - 2);
    e += e >= mn;
    e += e >= mx;
    const double gs = 1.2 + u01(q.z, q.w);
    const double* z = Z + (int64_t)e * ld;
    const double* z1 = Z + (int64_t)a * ld;
    const double* z2 = Z + (int64_t)c * ld;
    double pD = 0.0, pA = 0.0;
    for (int j = lane; j < P; j += 64) {
      const double d = xi[j] - z[j];
      const double dd = d * d;
      pD = pD + dd;
      const double g = z1[j] - z2[j];
      const double gd = g * d;
      pA = pA + gd;
    }
    const double D = zs_sum64(pD), A = zs_sum64(pA);
    if (D == 0.0 || !is_finite(D)) {  // a null move: the chain drew its own copy, or D is Inf or NaN
      // the trial row is left as an earlier generation wrote it, on purpose: active = 0 keeps every reader off it
      if (lane == 0) {
        pri[b] = qnan();
        ljac[b] = qnan();
        move[b] = 2;
        active[b] = 0;
      }
      return;  // the whole wavefront
    }
    const double r = A / D;
    const double s = gs * r;
    double pE = 0.0;
    for (int64_t j = lane; j < ld; j += 64) {
      double tj = xi[j];
      if (j < P) {
        const double zj = z[j];
        const double d = tj - zj;
        const double y = s * d;
        tj = tj + y;
        oob |= !(tj >= lo[j] && tj <= up[j]);  // a NaN fails both comparisons
        const double f = tj - zj;
        const double ff = f * f;
        pE = pE + ff;
      }
      tr[j] = tj;
    }
    const double Dp = zs_sum64(pE);
    const double h = 0.5 * (double)(P - 1);
    const double l1 = log(Dp), l0 = log(D);
    const double dl = l1 - l0;
    lj = h * dl;
  } else {
    const int jrand = (int)zs_scale(w.z, (uint32_t)P);
    const double* x1 = Z + (int64_t)a * ld;
    const double* x2 = Z + (int64_t)c * ld;
    const double* jit = jitter + (int64_t)k * ld;
    // pass 1: the two uniforms of every coordinate; the crossing flags stay in the mask, the jitter uniform is parked
    uint64_t mask = 0;
    int it = 0;
    for (int j = lane; j < P; j += 64, ++it) {
      const uint4 v = rng(seed, key, gen, kPurposeCoord, i * 4096u + (uint32_t)j);
      const double u = u01(v.x, v.y);
      if (jump || u < CR || j == jrand) mask |= (uint64_t)1 << it;
      tr[j] = u01(v.z, v.w);
    }
    int dcross = __popcll(mask);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) dcross += __shfl_xor(dcross, d, 64);  // integers: the order does not matter
    const double gam = jump ? 1.0 : gamma0 / sqrt((double)(2 * dcross));
    // pass 2: lane l reads back the uniforms it parked at j = l, l + 64, ..
    it = 0;
    for (int64_t j = lane; j < ld; j += 64, ++it) {
      double tj = xi[j];
      if (j < P && ((mask >> it) & 1)) {
        const double v = tr[j];
        const double d = x1[j] - x2[j];
        const double s = gam * d;
        const double y = tj + s;
        const double e2 = 2.0 * v;
        const double f = e2 - 1.0;
        const double zz = jit[j] * f;
        tj = y + zz;
        oob |= !(tj >= lo[j] && tj <= up[j]);
      }
      tr[j] = tj;
    }
  }
  const bool out = __ballot(oob) != 0;  // wave-uniform
  double tot = qnan();
  if (!out) tot = prior_sum64(tr, mu + (int64_t)k * ld, sig + (int64_t)k * ld, P, lane);  // its own stores
  if (lane == 0) {
    pri[b] = tot;
    ljac[b] = out && snk ? qnan() : lj;
    move[b] = snk ? 1 : 0;
    active[b] = out ? 0 : 1;
  }
}

// kInit: s2 and the counters of every chain and, when keep_row >= 0, kept row 0. Else: the decisions of generation gen,
// then the archive rows (app_row >= 0: the cell's archive row that chain 0 goes to) and the kept row.
template <bool kInit>
__global__ __launch_bounds__(kZsDecThreads) void k_zs_decide(
    const CellMeta* __restrict__ cells, const int32_t* __restrict__ cell_id, const int64_t* __restrict__ keys,
    const double* __restrict__ sigma2_0, const double* __restrict__ trial, const double* __restrict__ ss_t,
    const double* __restrict__ pri_t, const double* __restrict__ ljac, const uint8_t* __restrict__ move,
    const uint8_t* __restrict__ active, int n_pop, int64_t M_cap, int64_t ld, int64_t B, int64_t gen, uint64_t seed,
    int updatesigma, int64_t keep_row, int64_t app_row, int64_t log_row, double* pop, double* arch, double* ss, double* pri,
    double* s2, int32_t* __restrict__ n_acc, int32_t* __restrict__ n_oob, int32_t* __restrict__ n_null,
    double* __restrict__ chain, double* __restrict__ s2chain, double* __restrict__ sschain,
    double* __restrict__ prichain, double* __restrict__ logr, uint8_t* __restrict__ acc_log,
    uint8_t* __restrict__ oob_log, double* __restrict__ ljac_log, uint8_t* __restrict__ snk_log) {
  __shared__ uint8_t sh_take[kZsMaxPop];  // n_pop <= 4096 (the host checked)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t k = blockIdx.x;
  if (kInit) {
    const double s0 = sigma2_0[k];
    for (int i = threadIdx.x; i < n_pop; i += kZsDecThreads) {
      const int64_t b = k * n_pop + i;
      s2[b] = s0;
      n_acc[b] = 0;
      n_oob[b] = 0;
      n_null[b] = 0;
    }
  } else {
    const int64_t key = keys[k];
    const double shape = (double)cells[cell_id[k]].n;  // nobs / 2 with nobs = 2 N
    for (int i = threadIdx.x; i < n_pop; i += kZsDecThreads) {
      const int64_t b = k * n_pop + i;
      const bool act = active[b] != 0;
      const uint8_t mv = move[b];
      const double lj = ljac[b];
      const double s2i = s2[b];
      double ssi = ss[b], lr = qnan();
      bool take = false;
      if (act) {
        const double st = ss_t[b], pt = pri_t[b];
        const double qo = ssi / s2i;
        const double fo = qo + pri[b];  // formed afresh: s2 moves
        const double qn = st / s2i;
        const double fn = qn + pt;
        const double df = fn - fo;
        const double hl = -0.5 * df;
        lr = hl + lj;
        if (lr >= 0.0) {
          take = true;
        } else if (lr == lr) {  // a NaN logr rejects
          const uint4 r = rng(seed, key, gen, kPurposeAccept, (uint32_t)i);
          take = u01(r.x, r.y) < exp(lr);
        }
        if (take) {
          ss[b] = st;
          pri[b] = pt;
          ssi = st;
          n_acc[b] += 1;
        }
      } else if (mv == 2) {
        n_null[b] += 1;
      } else {
        n_oob[b] += 1;
      }
      if (updatesigma) {
        const double scale = 2.0 / ssi;
        const double g = gamma_unit_t(seed, key, gen, shape, kPurposeSigma, (uint32_t)i << 16);
        s2[b] = 1.0 / (g * scale);
      }
      sh_take[i] = take;
      if (log_row >= 0) {
        const int64_t at = log_row * B + b;
        if (logr) logr[at] = lr;
        if (acc_log) acc_log[at] = take;
        if (oob_log) oob_log[at] = act ? 0 : (mv == 2 ? 2 : 1);
        if (ljac_log) ljac_log[at] = lj;
        if (snk_log) snk_log[at] = mv != 0;
      }
    }
    __syncthreads();
    for (int i = wave; i < n_pop; i += kZsDecWaves)
      if (sh_take[i]) {  // wave-uniform
        const int64_t b = k * n_pop + i;
        for (int64_t j = lane; j < ld; j += 64) pop[b * ld + j] = trial[b * ld + j];
      }
  }
  if (keep_row < 0 && app_row < 0) return;  // kernel arguments: the whole workgroup
  __syncthreads();
  // the rows and values stored above are this workgroup's own stores, ordered by the barrier
  for (int i = wave; i < n_pop; i += kZsDecWaves) {
    const int64_t b = k * n_pop + i;
    if (app_row >= 0) {
      double* to = arch + (k * M_cap + app_row + i) * ld;
      for (int64_t j = lane; j < ld; j += 64) to[j] = pop[b * ld + j];
    }
    if (keep_row >= 0) {
      const int64_t at = keep_row * B + b;
      for (int64_t j = lane; j < ld; j += 64) chain[at * ld + j] = pop[b * ld + j];
      if (lane == 0) {
        s2chain[at] = s2[b];
        sschain[at] = ss[b];
        prichain[at] = pri[b];
      }
    }
  }
}

int zs_sizes(int64_t n_sel, int64_t n_pop, int64_t M_g, int64_t M_cap, int64_t ld, int64_t gen) {
  if (n_sel < 1 || n_pop < 1 || n_pop > kZsMaxPop || ld < 1 || gen < 0) return TCI_EINVAL;
  if (gen > 0 && (M_g < 3 || M_g > M_cap || M_cap >= ((int64_t)1 << 24))) return TCI_EINVAL;
  if ((long double)n_sel * (long double)n_pop > 2147483647.0L) return TCI_ERANGE;
  return TCI_OK;
}

}  // namespace

int launch_zs_propose(const KParams& kp, const int32_t* cell_id, const int64_t* keys, const double* pop,
                      const double* arch, const double* lower, const double* upper, const double* mu, const double* sig,
                      const double* jitter, int64_t n_sel, int64_t n_pop, int64_t M_g, int64_t M_cap, int64_t ld,
                      int64_t gen, bool jump, uint64_t seed, double gamma0, double CR, double p_snooker, double* trial,
                      double* pri, double* ljac, uint8_t* move, uint8_t* active, void* stream) {
  const int rc = zs_sizes(n_sel, n_pop, M_g, M_cap, ld, gen);
  if (rc != TCI_OK) return rc;
  if (!cell_id || !pop || !mu || !sig || !pri) return TCI_EINVAL;
  if (gen > 0 && (!keys || !arch || !lower || !upper || !jitter || !trial || !ljac || !move || !active)) return TCI_EINVAL;
  const int64_t B = n_sel * n_pop;
  const dim3 grid((unsigned)((B + kZsWaves - 1) / kZsWaves)), block(kZsThreads);
  if (gen == 0)
    hipLaunchKernelGGL(k_zs_propose<true>, grid, block, 0, (hipStream_t)stream, kp.cells, cell_id, keys, pop, arch, lower,
                       upper, mu, sig, jitter, (uint32_t)n_pop, (uint32_t)M_g, M_cap, ld, B, gen, (int)jump, seed, gamma0, CR,
                       p_snooker, trial, pri, ljac, move, active);
  else
    hipLaunchKernelGGL(k_zs_propose<false>, grid, block, 0, (hipStream_t)stream, kp.cells, cell_id, keys, pop, arch, lower,
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
                     uint8_t* oob_log, double* ljac_log, uint8_t* snk_log, void* stream) {
  const int rc = zs_sizes(n_sel, n_pop, 3, M_cap, ld, 0);
  if (rc != TCI_OK) return rc;
  if (!cell_id || !sigma2_0 || !pop || !ss || !pri || !s2 || !n_acc || !n_oob || !n_null) return TCI_EINVAL;
  if (gen > 0 && (!keys || !trial || !ss_t || !pri_t || !ljac || !move || !active)) return TCI_EINVAL;
  if (keep_row >= 0 && (!chain || !s2chain || !sschain || !prichain)) return TCI_EINVAL;
  if (app_row >= 0 && (!arch || app_row + n_pop > M_cap)) return TCI_EINVAL;
  const int64_t B = n_sel * n_pop;
  const dim3 grid((unsigned)n_sel), block(kZsDecThreads);
  if (gen == 0)
    hipLaunchKernelGGL(k_zs_decide<true>, grid, block, 0, (hipStream_t)stream, kp.cells, cell_id, keys, sigma2_0, trial,
                       ss_t, pri_t, ljac, move, active, (int)n_pop, M_cap, ld, B, gen, seed, (int)updatesigma, keep_row,
                       app_row, log_row, pop, arch, ss, pri, s2, n_acc, n_oob, n_null, chain, s2chain, sschain, prichain, logr,
                       acc_log, oob_log, ljac_log, snk_log);
  else
    hipLaunchKernelGGL(k_zs_decide<false>, grid, block, 0, (hipStream_t)stream, kp.cells, cell_id, keys, sigma2_0, trial,
                       ss_t, pri_t, ljac, move, active, (int)n_pop, M_cap, ld, B, gen, seed, (int)updatesigma, keep_row,
                       app_row, log_row, pop, arch, ss, pri, s2, n_acc, n_oob, n_null, chain, s2chain, sschain, prichain, logr,
                       acc_log, oob_log, ljac_log, snk_log);
  return hipGetLastError() == hipSuccess ? TCI_OK : TCI_EHIP;
}

}  // namespace tci
