// tci_modesearch.hip -- differential evolution (DE/rand/1/bin, Storn and Price 1997) over a population of theta rows
// per cell, ahead of the sampler: a global search for a good mode of f = ss / s2 + pri. The definition is in
// include/tci.h (tci_modesearch).
//
// The population lies as [n_sel][n_pop][ld]; row b = k * n_pop + i is member i of selected cell k, and f, ss and pri are
// laid out as the rows are. A generation is three launches on one stream:
//   k_ms_trial   one wavefront per (cell, member): every lane draws the member's index quadruple (r1, r2, r3, jrand) from
//                the same Philox call, then the lanes stride over the coordinates j = lane, lane + 64, ..: the
//                crossover uniform of j, the mutant, the bounds test, the trial entry. The lanes then sum the trial's
//                prior in tci_chainlp's 64-partial order (tci_prior.h): lane l reads back exactly the entries it wrote.
//                Generation 0 (kInit): the prior of the member itself, nothing else.
//   (the batched likelihood kernel, tci_kernels.hip, on the trial buffer, every row active: launched by the host entry)
//   k_ms_select  one workgroup per cell. A thread per member forms f_trial, decides and stores the member's values, with
//                its f after the generation and the decision in LDS; after the barrier the waves stride over the
//                members and copy every accepted trial over its parent, and wave 0 scans the LDS copy for the least f
//                (the least index among equals), which gives best and the trace entry, and counts the decisions. On
//                the last generation the workgroup also writes the best member's row and values. Generation 0 (kInit):
//                f of every member, no copy.
// All members of a generation read the population as the previous generation's selection left it (synchronous DE): the
// trial kernel only reads it, the selection kernel only writes it, and the launches are ordered by the stream.
// Bits: a row's trial depends on the cell's population, bounds, key, seed, generation and member index alone; the scan
// is a minimum under a total order, so the split over lanes does not matter. Every loop is bounded by an integer count.
#include <hip/hip_runtime.h>

#include "tci_fp.h"
#include "tci_internal.h"
#include "tci_prior.h"
#include "tci_rng.h"

namespace tci {

namespace {

constexpr int kMsThreads = 256;
constexpr int kMsWaves = kMsThreads / 64;
constexpr int kMsSelThreads = 1024;  // k_ms_select: one workgroup per cell
constexpr int kMsSelWaves = kMsSelThreads / 64;
constexpr uint32_t kPurposeIndex = 7, kPurposeCross = 8;  // 1-6 are the sampler's (tci_dram.hip)
// the crossover counter i * 2048 + (j >> 1) is one per (member, coordinate pair) while j < 4096; tci_create admits no
// longer cell
static_assert(7 + TCI_MAX_POINTS <= 4096, "the crossover counter of k_ms_trial");

// m(w, n) of include/tci.h: a word scaled to [0, n)
__device__ __forceinline__ uint32_t ms_scale(uint32_t w, uint32_t n) { return (uint32_t)(((uint64_t)w * n) >> 32); }

// (a before b) in the order the scan minimises: a NaN after every number, equal values by index
__device__ __forceinline__ bool ms_before(double fa, int ia, double fb, int ib) {
  const bool na = fa != fa, nb = fb != fb;
  if (na != nb) return nb;
  if (!na && fa != fb) return fa < fb;
  return ia < ib;
}

template <bool kInit>
__global__ __launch_bounds__(kMsThreads) void k_ms_trial(const CellMeta* __restrict__ cells,
                                                          const int32_t* __restrict__ cell_id,
                                                          const int64_t* __restrict__ keys, const double* __restrict__ pop,
                                                          const double* __restrict__ lower, const double* __restrict__ upper,
                                                          const double* __restrict__ mu, const double* __restrict__ sig,
                                                          uint32_t n_pop, int64_t ld, int64_t B, int64_t gen, uint64_t seed,
                                                          double F, double CR, double* trial, double* __restrict__ pri) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.x * kMsWaves + wave;
  if (b >= B) return;  // the whole wavefront
  const uint32_t k = (uint32_t)b / n_pop, i = (uint32_t)b % n_pop;  // B < 2^31 (the host checked): 32-bit divisions
  const int P = 7 + cells[cell_id[k]].n;                            // <= ld (the host checked)
  const double* m = mu + (int64_t)k * ld;
  const double* sg = sig + (int64_t)k * ld;
  if (kInit) {
    const double tot = prior_sum64(pop + b * ld, m, sg, P, lane);
    if (lane == 0) pri[b] = tot;
    return;
  }
  const int64_t key = keys[k];
  const uint4 w = rng(seed, key, gen, kPurposeIndex, i);
  uint32_t r1 = ms_scale(w.x, n_pop - 1);
  r1 += r1 >= i;
  const uint32_t a2 = i < r1 ? i : r1, b2 = i < r1 ? r1 : i;  // {i, r1} ascending
  uint32_t r2 = ms_scale(w.y, n_pop - 2);
  r2 += r2 >= a2;
  r2 += r2 >= b2;
  // {i, r1, r2} ascending: r2 goes below, between or above the pair
  const uint32_t a3 = r2 < a2 ? r2 : a2, c3 = r2 > b2 ? r2 : b2, b3 = r2 < a2 ? a2 : (r2 > b2 ? b2 : r2);
  uint32_t r3 = ms_scale(w.z, n_pop - 3);
  r3 += r3 >= a3;
  r3 += r3 >= b3;
  r3 += r3 >= c3;
  const int jrand = (int)ms_scale(w.w, (uint32_t)P);
  const int64_t row0 = (int64_t)k * n_pop;
  const double* xi = pop + b * ld;
  const double* x1 = pop + (row0 + r1) * ld;
  const double* x2 = pop + (row0 + r2) * ld;
  const double* x3 = pop + (row0 + r3) * ld;
  const double* lo = lower + (int64_t)k * ld;
  const double* up = upper + (int64_t)k * ld;
  double* t = trial + b * ld;
  for (int64_t j = lane; j < ld; j += 64) {
    double tj = xi[j];
    if (j < P) {
      const uint4 c = rng(seed, key, gen, kPurposeCross, i * 2048u + (uint32_t)(j >> 1));
      const double u = (j & 1) ? u01(c.z, c.w) : u01(c.x, c.y);
      const double d = x2[j] - x3[j];
      const double s = F * d;
      const double v = x1[j] + s;
      // a NaN mutant fails both comparisons and keeps the parent's entry
      if ((u < CR || j == jrand) && v >= lo[j] && v <= up[j]) tj = v;
    }
    t[j] = tj;
  }
  const double tot = prior_sum64(t, m, sg, P, lane);  // lane l reads the entries j = l, l + 64, .. it stored itself
  if (lane == 0) pri[b] = tot;
}

template <bool kInit>
__global__ __launch_bounds__(kMsSelThreads) void k_ms_select(const CellMeta* __restrict__ cells,
                                                           const int32_t* __restrict__ cell_id,
                                                           const double* __restrict__ s2, const double* __restrict__ trial,
                                                           const double* __restrict__ ss_t, const double* __restrict__ pri_t,
                                                           int n_pop, int64_t ld, int final_gen, double* pop, double* f,
                                                           double* ss, double* pri, double* __restrict__ f_trace,
                                                           int32_t* __restrict__ n_acc, int32_t* __restrict__ best,
                                                           double* __restrict__ best_vals, double* __restrict__ theta_best,
                                                           int64_t n_sel) {
  __shared__ double sh_f[4096];  // n_pop <= 4096 (the host checked)
  __shared__ uint8_t sh_take[4096];
  __shared__ int sh_best;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t k = blockIdx.x;
  const double sk = s2[k];
  // one thread per member: the objective, the decision and the member's values (the loads of all members in flight
  // at once); the rows follow below
  for (int i = threadIdx.x; i < n_pop; i += kMsSelThreads) {
    const int64_t b = k * n_pop + i;
    if (kInit) {
      const double a = ss[b] / sk;
      const double fi = a + pri[b];
      f[b] = fi;
      sh_f[i] = fi;
      sh_take[i] = 0;
    } else {
      const double st = ss_t[b], pt = pri_t[b];
      const double a = st / sk;
      const double ft = a + pt;
      const double fp = f[b];
      const bool take = ft <= fp;  // a NaN f_trial never replaces
      if (take) {
        f[b] = ft;
        ss[b] = st;
        pri[b] = pt;
      }
      sh_f[i] = take ? ft : fp;
      sh_take[i] = take;
    }
  }
  __syncthreads();
  if (!kInit)
    for (int i = wave; i < n_pop; i += kMsSelWaves)
      if (sh_take[i]) {  // wave-uniform
        const int64_t b = k * n_pop + i;
        for (int64_t j = lane; j < ld; j += 64) pop[b * ld + j] = trial[b * ld + j];
      }
  if (wave == 0) {
    double bf = sh_f[0];
    int bi = 0, acc = 0;
    for (int i = lane; i < n_pop; i += 64) {
      const double x = sh_f[i];
      acc += sh_take[i];
      if (ms_before(x, i, bf, bi)) {
        bf = x;
        bi = i;
      }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const double of = __shfl_xor(bf, d, 64);
      const int oi = __shfl_xor(bi, d, 64);
      acc += __shfl_xor(acc, d, 64);
      if (ms_before(of, oi, bf, bi)) {
        bf = of;
        bi = oi;
      }
    }
    if (lane == 0) {
      sh_best = bi;
      f_trace[k] = bf;
      best[k] = bi;
      if (!kInit) n_acc[k] = acc;
    }
  }
  if (!final_gen) return;  // kernel argument: the whole workgroup
  __syncthreads();
  // the rows and values the selection above stored are this workgroup's own stores, ordered by the barrier
  const int64_t bb = k * n_pop + sh_best;
  const int P = 7 + cells[cell_id[k]].n;
  const double nan = qnan();
  for (int64_t j = threadIdx.x; j < ld; j += kMsSelThreads) theta_best[k * ld + j] = j < P ? pop[bb * ld + j] : nan;
  if (threadIdx.x == 0) {
    best_vals[k] = f[bb];
    best_vals[n_sel + k] = ss[bb];
    best_vals[2 * n_sel + k] = pri[bb];
  }
}

}  // namespace

int launch_modesearch_trial(const KParams& kp, const int32_t* cell_id, const int64_t* keys, const double* pop,
                            const double* lower, const double* upper, const double* mu, const double* sig, int64_t n_sel,
                            int64_t n_pop, int64_t ld, int64_t gen, uint64_t seed, double F, double CR, double* trial,
                            double* pri, void* stream) {
  if (n_sel < 1 || n_pop < 4 || n_pop > 4096 || ld < 1 || gen < 0) return TCI_EINVAL;
  if ((long double)n_sel * (long double)n_pop > 2147483647.0L) return TCI_ERANGE;
  if (!cell_id || !pop || !mu || !sig || !pri) return TCI_EINVAL;
  if (gen > 0 && (!keys || !lower || !upper || !trial)) return TCI_EINVAL;
  const int64_t B = n_sel * n_pop;
  const dim3 grid((unsigned)((B + kMsWaves - 1) / kMsWaves)), block(kMsThreads);
  if (gen == 0)
    hipLaunchKernelGGL(k_ms_trial<true>, grid, block, 0, (hipStream_t)stream, kp.cells, cell_id, keys, pop, lower, upper, mu,
                       sig, (uint32_t)n_pop, ld, B, gen, seed, F, CR, trial, pri);
  else
    hipLaunchKernelGGL(k_ms_trial<false>, grid, block, 0, (hipStream_t)stream, kp.cells, cell_id, keys, pop, lower, upper,
                       mu, sig, (uint32_t)n_pop, ld, B, gen, seed, F, CR, trial, pri);
  return hipGetLastError() == hipSuccess ? TCI_OK : TCI_EHIP;
}

int launch_modesearch_select(const KParams& kp, const int32_t* cell_id, const double* s2, const double* trial,
                             const double* ss_t, const double* pri_t, int64_t n_sel, int64_t n_pop, int64_t ld, int64_t gen,
                             bool final_gen, double* pop, double* f, double* ss, double* pri, double* f_trace,
                             int32_t* n_acc, int32_t* best, double* best_vals, double* theta_best, void* stream) {
  if (n_sel < 1 || n_pop < 4 || n_pop > 4096 || ld < 1 || gen < 0) return TCI_EINVAL;
  if ((long double)n_sel * (long double)n_pop > 2147483647.0L) return TCI_ERANGE;
  if (!cell_id || !s2 || !pop || !f || !ss || !pri || !f_trace || !best || !best_vals || !theta_best) return TCI_EINVAL;
  if (gen > 0 && (!trial || !ss_t || !pri_t || !n_acc)) return TCI_EINVAL;
  const dim3 grid((unsigned)n_sel), block(kMsSelThreads);
  if (gen == 0)
    hipLaunchKernelGGL(k_ms_select<true>, grid, block, 0, (hipStream_t)stream, kp.cells, cell_id, s2, trial, ss_t, pri_t,
                       (int)n_pop, ld, (int)final_gen, pop, f, ss, pri, f_trace, n_acc, best, best_vals, theta_best, n_sel);
  else
    hipLaunchKernelGGL(k_ms_select<false>, grid, block, 0, (hipStream_t)stream, kp.cells, cell_id, s2, trial, ss_t, pri_t,
                       (int)n_pop, ld, (int)final_gen, pop, f, ss, pri, f_trace, n_acc, best, best_vals, theta_best, n_sel);
  return hipGetLastError() == hipSuccess ? TCI_OK : TCI_EHIP;
}

}  // namespace tci
