// tci_demc.hip -- differential-evolution Markov chain (DE-MC, ter Braak 2006) over a population of theta rows per cell:
// a sampler beside DRAM whose proposal is the difference of two other members of the same cell, so that it needs no
// covariance adaptation. The definition is in include/tci.h (tci_demc_run).
//
// The population lies as [n_sel][n_pop][ld]; row b = k * n_pop + i is member i of selected cell k, and ss, pri, s2 and
// the counters are laid out as the rows are. A generation is two half-sweeps; in half-sweep h the members with
// i mod 2 == h move and take their pair from the other half, which rests. A half-sweep is three launches on one stream:
//   k_demc_propose  one wavefront per MOVING member. Every lane draws the member's (r1, r2, jrand) from the same Philox
//                   call, then the lanes stride over the coordinates j = lane, lane + 64, .. twice. Pass 1: one Philox
//                   call per coordinate gives the crossover uniform and the jitter uniform; the lane keeps the crossing
//                   flags of its (at most 33) coordinates in a 64-bit mask and parks the jitter uniform in the trial
//                   entry it will overwrite. An integer wave sum of the mask's population counts is d', which fixes
//                   gamma. Pass 2: the lane reads its parked uniform back, forms the trial entry and tests the bounds.
//                   A row with a crossing entry out of bounds gets active = 0 and no prior; any other row's prior is
//                   summed in tci_chainlp's 64-partial order (tci_prior.h) by the lanes that wrote the entries.
//   (the batched likelihood kernel, tci_kernels.hip, on the trial buffer under the active mask: launched by the host)
//   k_demc_decide   one workgroup per cell. A thread per moving member forms logr, decides, draws the member's sigma2
//                   and stores its values, with the decision in LDS; after the barrier the waves stride over the moving
//                   members and copy every accepted trial over its parent; on a kept generation (after half-sweep 1)
//                   a second barrier, then the waves stride over ALL members and store the kept row.
// Shapes, and what differs from the mode search. The trial buffer, its ss, pri and active vectors hold
// the moving members alone, row t = k * n_mov + (i >> 1): the likelihood launch of a half-sweep has n_sel * n_mov rows,
// so a resting row costs it nothing at all, not even the inactive-row path. The mode search's trial kernel spent its time
// in one Philox call per lane and coordinate with neighbouring lanes repeating each other's call; here a call serves one
// coordinate's two uniforms, no lane repeats another's, and pass 2 runs no generator at all.
// Bits: a member's trial depends on the cell's population, bounds, jitter, key, seed, generation, half-sweep and member
// index alone; d' is an integer sum. Every loop is bounded by an integer count.
#include <hip/hip_runtime.h>
#include <math.h>

#include "tci_fp.h"
#include "tci_gamma.h"
#include "tci_internal.h"
#include "tci_prior.h"
#include "tci_rng.h"

namespace tci {

namespace {

constexpr int kDmThreads = 256;
constexpr int kDmWaves = kDmThreads / 64;
constexpr int kDmDecThreads = 1024;  // k_demc_decide: one workgroup per cell
constexpr int kDmDecWaves = kDmDecThreads / 64;
// 1-6 are the sampler's (tci_dram.hip), 7 and 8 the mode search's (tci_modesearch.hip)
constexpr uint32_t kPurposeIndex = 9, kPurposeCoord = 10, kPurposeAccept = 11, kPurposeSigma = 12;
// the coordinate counter i * 4096 + j is one per (member, coordinate) while j < 4096 and i < 4096 (i * 4096 + j < 2^24);
// tci_create admits no longer cell and the host no larger population
static_assert(7 + TCI_MAX_POINTS <= 4096, "the coordinate counter of k_demc_propose");
// a lane's crossing flags, one bit per stride of 64 coordinates
static_assert((7 + TCI_MAX_POINTS + 63) / 64 <= 64, "the crossing mask of k_demc_propose");

// m(w, n) of include/tci.h: a word scaled to [0, n)
__device__ __forceinline__ uint32_t dm_scale(uint32_t w, uint32_t n) { return (uint32_t)(((uint64_t)w * n) >> 32); }

// kInit: the prior of every member of pop, one wavefront per member (B = n_sel * n_pop rows). Else: the trial of every
// moving member of half-sweep h (B = n_sel * n_mov rows).
template <bool kInit>
__global__ __launch_bounds__(kDmThreads) void k_demc_propose(
    const CellMeta* __restrict__ cells, const int32_t* __restrict__ cell_id, const int64_t* __restrict__ keys,
    const double* __restrict__ pop, const double* __restrict__ lower, const double* __restrict__ upper,
    const double* __restrict__ mu, const double* __restrict__ sig, const double* __restrict__ jitter, uint32_t n_pop,
    uint32_t n_mov, int64_t ld, int64_t B, int64_t gen, uint32_t h, int jump, uint64_t seed, double gamma0, double CR,
    double* trial, double* __restrict__ pri, uint8_t* __restrict__ active) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t t = (int64_t)blockIdx.x * kDmWaves + wave;
  if (t >= B) return;  // the whole wavefront
  if (kInit) {
    const uint32_t k = (uint32_t)t / n_pop;  // B < 2^31 (the host checked): 32-bit divisions
    const int P = 7 + cells[cell_id[k]].n;   // <= ld (the host checked)
    const double tot = prior_sum64(pop + t * ld, mu + (int64_t)k * ld, sig + (int64_t)k * ld, P, lane);
    if (lane == 0) pri[t] = tot;
    return;
  }
  const uint32_t k = (uint32_t)t / n_mov, i = 2u * ((uint32_t)t % n_mov) + h;
  const int P = 7 + cells[cell_id[k]].n;
  const int64_t key = keys[k], step = 2 * gen + (int64_t)h;
  const uint32_t n_rest = n_pop - n_mov;  // >= 2: n_pop >= 4
  const uint4 w = rng(seed, key, step, kPurposeIndex, i);
  const uint32_t a = dm_scale(w.x, n_rest);
  uint32_t c = dm_scale(w.y, n_rest - 1);
  c += c >= a;
  const uint32_t r1 = 2u * a + (1u - h), r2 = 2u * c + (1u - h);  // the resting members, ascending: 1 - h, 3 - h, ..
  const int jrand = (int)dm_scale(w.z, (uint32_t)P);
  const int64_t row0 = (int64_t)k * n_pop;
  const double* xi = pop + (row0 + i) * ld;
  const double* x1 = pop + (row0 + r1) * ld;
  const double* x2 = pop + (row0 + r2) * ld;
  const double* lo = lower + (int64_t)k * ld;
  const double* up = upper + (int64_t)k * ld;
  const double* jit = jitter + (int64_t)k * ld;
  double* tr = trial + t * ld;
  // pass 1: the two uniforms of every coordinate; the crossing flags stay in the mask, the jitter uniform is parked
  uint64_t mask = 0;
  int it = 0;
  for (int j = lane; j < P; j += 64, ++it) {
    const uint4 q = rng(seed, key, step, kPurposeCoord, i * 4096u + (uint32_t)j);
    const double u = u01(q.x, q.y);
    if (jump || u < CR || j == jrand) mask |= (uint64_t)1 << it;
    tr[j] = u01(q.z, q.w);
  }
  int dcross = __popcll(mask);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) dcross += __shfl_xor(dcross, d, 64);  // integers: the order does not matter
  // d' >= 1 (jrand crosses); sqrt and the division are the correctly rounded ones
  const double gam = jump ? 1.0 : gamma0 / sqrt((double)(2 * dcross));
  // pass 2: lane l reads back the uniforms it parked at j = l, l + 64, ..
  bool oob = false;
  it = 0;
  for (int64_t j = lane; j < ld; j += 64, ++it) {
    double tj = xi[j];
    if (j < P && ((mask >> it) & 1)) {
      const double v = tr[j];
      const double d = x1[j] - x2[j];
      const double s = gam * d;
      const double y = tj + s;
      const double e = 2.0 * v;
      const double f = e - 1.0;
      const double z = jit[j] * f;
      tj = y + z;
      oob |= !(tj >= lo[j] && tj <= up[j]);  // a NaN fails both comparisons
    }
    tr[j] = tj;
  }
  const bool out = __ballot(oob) != 0;  // wave-uniform
  double tot = qnan();
  if (!out) tot = prior_sum64(tr, mu + (int64_t)k * ld, sig + (int64_t)k * ld, P, lane);  // its own stores, as above
  if (lane == 0) {
    pri[t] = tot;
    active[t] = out ? 0 : 1;
  }
}

// kInit: s2 and the counters of every member and, when keep_row >= 0, kept row 0. Else: the decisions of half-sweep h.
template <bool kInit>
__global__ __launch_bounds__(kDmDecThreads) void k_demc_decide(
    const CellMeta* __restrict__ cells, const int32_t* __restrict__ cell_id, const int64_t* __restrict__ keys,
    const double* __restrict__ sigma2_0, const double* __restrict__ trial, const double* __restrict__ ss_t,
    const double* __restrict__ pri_t, const uint8_t* __restrict__ active, int n_pop, int n_mov, int64_t ld, int64_t B,
    int64_t gen, int h, uint64_t seed, int updatesigma, int64_t keep_row, int64_t log_row, double* pop, double* ss,
    double* pri, double* s2, int32_t* __restrict__ n_acc, int32_t* __restrict__ n_oob, double* __restrict__ chain,
    double* __restrict__ s2chain, double* __restrict__ sschain, double* __restrict__ prichain,
    double* __restrict__ logr, uint8_t* __restrict__ acc_log, uint8_t* __restrict__ oob_log) {
  __shared__ uint8_t sh_take[2048];  // n_mov <= 2048 (the host checked n_pop <= 4096)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t k = blockIdx.x;
  if (kInit) {
    const double s0 = sigma2_0[k];
    for (int i = threadIdx.x; i < n_pop; i += kDmDecThreads) {
      const int64_t b = k * n_pop + i;
      s2[b] = s0;
      n_acc[b] = 0;
      n_oob[b] = 0;
    }
  } else {
    const int64_t key = keys[k], step = 2 * gen + h;
    const double shape = (double)cells[cell_id[k]].n;  // nobs / 2 with nobs = 2 N
    // one thread per moving member: the loads of all members in flight at once; the rows follow below
    for (int mi = threadIdx.x; mi < n_mov; mi += kDmDecThreads) {
      const int i = 2 * mi + h;
      const int64_t b = k * n_pop + i, t = k * n_mov + mi;
      const bool act = active[t] != 0;
      const double s2i = s2[b];
      double ssi = ss[b], lr = qnan();
      bool take = false;
      if (act) {
        const double st = ss_t[t], pt = pri_t[t];
        const double qo = ssi / s2i;
        const double fo = qo + pri[b];  // formed afresh: s2 moves
        const double qn = st / s2i;
        const double fn = qn + pt;
        const double df = fn - fo;
        lr = -0.5 * df;
        if (lr >= 0.0) {
          take = true;
        } else if (lr == lr) {  // a NaN logr rejects
          const uint4 r = rng(seed, key, step, kPurposeAccept, (uint32_t)i);
          take = u01(r.x, r.y) < exp(lr);
        }
        if (take) {
          ss[b] = st;
          pri[b] = pt;
          ssi = st;
          n_acc[b] += 1;
        }
      } else {
        n_oob[b] += 1;
      }
      if (updatesigma) {
        const double scale = 2.0 / ssi;
        const double g = gamma_unit_t(seed, key, step, shape, kPurposeSigma, (uint32_t)i << 16);
        s2[b] = 1.0 / (g * scale);
      }
      sh_take[mi] = take;
      if (log_row >= 0) {
        const int64_t at = log_row * B + b;
        if (logr) logr[at] = lr;
        if (acc_log) acc_log[at] = take;
        if (oob_log) oob_log[at] = !act;
      }
    }
    __syncthreads();
    for (int mi = wave; mi < n_mov; mi += kDmDecWaves)
      if (sh_take[mi]) {  // wave-uniform
        const int64_t b = k * n_pop + 2 * mi + h, t = k * n_mov + mi;
        for (int64_t j = lane; j < ld; j += 64) pop[b * ld + j] = trial[t * ld + j];
      }
  }
  if (keep_row < 0) return;  // kernel argument: the whole workgroup
  __syncthreads();
  // the rows and values stored above are this workgroup's own stores, ordered by the barrier
  for (int i = wave; i < n_pop; i += kDmDecWaves) {
    const int64_t b = k * n_pop + i, at = keep_row * B + b;
    for (int64_t j = lane; j < ld; j += 64) chain[at * ld + j] = pop[b * ld + j];
    if (lane == 0) {
      s2chain[at] = s2[b];
      sschain[at] = ss[b];
      prichain[at] = pri[b];
    }
  }
}

int demc_sizes(int64_t n_sel, int64_t n_pop, int64_t ld, int64_t gen, int h) {
  if (n_sel < 1 || n_pop < 4 || n_pop > 4096 || ld < 1 || gen < 0 || h < 0 || h > 1) return TCI_EINVAL;
  if ((long double)n_sel * (long double)n_pop > 2147483647.0L) return TCI_ERANGE;
  return TCI_OK;
}

}  // namespace

int launch_demc_propose(const KParams& kp, const int32_t* cell_id, const int64_t* keys, const double* pop,
                        const double* lower, const double* upper, const double* mu, const double* sig,
                        const double* jitter, int64_t n_sel, int64_t n_pop, int64_t ld, int64_t gen, int h, bool jump,
                        uint64_t seed, double gamma0, double CR, double* trial, double* pri, uint8_t* active,
                        void* stream) {
  const int rc = demc_sizes(n_sel, n_pop, ld, gen, h);
  if (rc != TCI_OK) return rc;
  if (!cell_id || !pop || !mu || !sig || !pri) return TCI_EINVAL;
  if (gen > 0 && (!keys || !lower || !upper || !jitter || !trial || !active)) return TCI_EINVAL;
  const int64_t n_mov = (n_pop - h + 1) / 2;
  const int64_t B = gen == 0 ? n_sel * n_pop : n_sel * n_mov;
  const dim3 grid((unsigned)((B + kDmWaves - 1) / kDmWaves)), block(kDmThreads);
  if (gen == 0)
    hipLaunchKernelGGL(k_demc_propose<true>, grid, block, 0, (hipStream_t)stream, kp.cells, cell_id, keys, pop, lower,
                       upper, mu, sig, jitter, (uint32_t)n_pop, (uint32_t)n_mov, ld, B, gen, (uint32_t)h, (int)jump, seed,
                       gamma0, CR, trial, pri, active);
  else
    hipLaunchKernelGGL(k_demc_propose<false>, grid, block, 0, (hipStream_t)stream, kp.cells, cell_id, keys, pop, lower,
                       upper, mu, sig, jitter, (uint32_t)n_pop, (uint32_t)n_mov, ld, B, gen, (uint32_t)h, (int)jump, seed,
                       gamma0, CR, trial, pri, active);
  return hipGetLastError() == hipSuccess ? TCI_OK : TCI_EHIP;
}

int launch_demc_decide(const KParams& kp, const int32_t* cell_id, const int64_t* keys, const double* sigma2_0,
                       const double* trial, const double* ss_t, const double* pri_t, const uint8_t* active,
                       int64_t n_sel, int64_t n_pop, int64_t ld, int64_t gen, int h, uint64_t seed, bool updatesigma,
                       int64_t keep_row, int64_t log_row, double* pop, double* ss, double* pri, double* s2,
                       int32_t* n_acc, int32_t* n_oob, double* chain, double* s2chain, double* sschain,
                       double* prichain, double* logr, uint8_t* acc_log, uint8_t* oob_log, void* stream) {
  const int rc = demc_sizes(n_sel, n_pop, ld, gen, h);
  if (rc != TCI_OK) return rc;
  if (!cell_id || !sigma2_0 || !pop || !ss || !pri || !s2 || !n_acc || !n_oob) return TCI_EINVAL;
  if (gen > 0 && (!keys || !trial || !ss_t || !pri_t || !active)) return TCI_EINVAL;
  if (keep_row >= 0 && (!chain || !s2chain || !sschain || !prichain)) return TCI_EINVAL;
  const int64_t n_mov = (n_pop - h + 1) / 2, B = n_sel * n_pop;
  const dim3 grid((unsigned)n_sel), block(kDmDecThreads);
  if (gen == 0)
    hipLaunchKernelGGL(k_demc_decide<true>, grid, block, 0, (hipStream_t)stream, kp.cells, cell_id, keys, sigma2_0, trial,
                       ss_t, pri_t, active, (int)n_pop, (int)n_mov, ld, B, gen, h, seed, (int)updatesigma, keep_row,
                       log_row, pop, ss, pri, s2, n_acc, n_oob, chain, s2chain, sschain, prichain, logr, acc_log, oob_log);
  else
    hipLaunchKernelGGL(k_demc_decide<false>, grid, block, 0, (hipStream_t)stream, kp.cells, cell_id, keys, sigma2_0,
                       trial, ss_t, pri_t, active, (int)n_pop, (int)n_mov, ld, B, gen, h, seed, (int)updatesigma, keep_row,
                       log_row, pop, ss, pri, s2, n_acc, n_oob, chain, s2chain, sschain, prichain, logr, acc_log, oob_log);
  return hipGetLastError() == hipSuccess ? TCI_OK : TCI_EHIP;
}

}  // namespace tci
