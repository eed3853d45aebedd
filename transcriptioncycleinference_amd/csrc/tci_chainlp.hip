// tci_chainlp.hip -- the sum-of-squares, prior, deviance and log-posterior trace of every chain (mcmcstat's sschain),
// its best sample and DIC, reduced on the device; the definition is in include/tci.h.
//
// The chain lies as [rows][n_chains][ld], its s2 as [rows][n_chains]; row b = t * n_chains + c of either is row t of
// chain c, and the four traces (ss, pri, dev, lp) are laid out as s2 is. The SS trace is the batched likelihood
// kernel's (tci_kernels.hip), launched by the caller straight on the chain with the cell-id vector k_chainlp_ids
// writes, so it is the SS the sampler saw.
//
//   k_chainlp_ids     the cell id of every (row, chain).
//   k_chainlp_rows    one wavefront per (row, chain): lane l sums the prior terms j = l, l + 64, .. in ascending j, the
//                     64 partials are added in ascending lane order by every lane alike (tci_prior.h); lane 0 then
//                     forms dev and lp.
//   k_chainlp_reduce  one workgroup per chain. The rows are cut into segments of kLpSeg rows (the count and the
//                     boundaries follow from n alone); a thread reduces whole segments, row by row in order, and
//                     stores every segment's partial results; thread 0 adds them in segment order. A second pass
//                     over the segments gives the centred sum of squares of dev. The best row is the first row of
//                     the largest lp: a segment keeps its first, the segments are compared in order with >.
// An output's bits depend on the chain's rows, its s2, cell and priors and on n alone, never on n_chains, on where
// the chain sits, on ld or on how many workgroups ran. Every loop is bounded by an integer count.
#include <hip/hip_runtime.h>

#include <cmath>

#include "tci_fp.h"
#include "tci_internal.h"
#include "tci_prior.h"

namespace tci {

namespace {

constexpr int kLpSeg = 256;      // rows per segment
constexpr int kLpWaves = 4;      // k_chainlp_rows: (row, chain) pairs per workgroup, one per wavefront
constexpr int kLpThreads = 256;
constexpr int kLpSegVals = 4;    // doubles a segment stores: sum ss (pass 2: the centred squares), sum dev, min ss, max lp

// dev of include/tci.h: ss / s2 + nobs * log(2 pi s2), every operation rounded once
__device__ __forceinline__ double lp_deviance(double ss, double s2, double nobs) {
  const double a = ss / s2;
  const double b = 6.283185307179586 * s2;
  const double d = nobs * log(b);
  return a + d;
}

__global__ __launch_bounds__(kLpThreads) void k_chainlp_ids(const int32_t* __restrict__ cell, int64_t n_chains, int64_t B,
                                                             int32_t* __restrict__ row_cell) {
  const int64_t b = (int64_t)blockIdx.x * kLpThreads + threadIdx.x;
  if (b < B) row_cell[b] = cell[(uint32_t)b % (uint32_t)n_chains];  // B < 2^31 (lp_sizes): a 32-bit division
}

__global__ __launch_bounds__(kLpThreads) void k_chainlp_rows(const CellMeta* __restrict__ cells,
                                                              const double* __restrict__ chain,
                                                              const double* __restrict__ s2, const double* __restrict__ ss,
                                                              const int32_t* __restrict__ cell,
                                                              const double* __restrict__ mu, const double* __restrict__ sig,
                                                              int64_t n_chains, int64_t ld, int64_t B,
                                                              double* __restrict__ pri, double* __restrict__ dev,
                                                              double* __restrict__ lp) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.x * kLpWaves + wave;
  if (b >= B) return;  // the whole wavefront
  const int64_t c = (uint32_t)b % (uint32_t)n_chains;  // B < 2^31 (lp_sizes): a 32-bit division
  const int N = cells[cell[c]].n;
  const int P = 7 + N;  // <= ld (the host checked)
  const double* th = chain + b * ld;
  const double* m = mu + c * ld;
  const double* sg = sig + c * ld;
  const double tot = prior_sum64(th, m, sg, P, lane);
  if (lane == 0) {
    const double d = lp_deviance(ss[b], s2[b], (double)(2 * N));
    pri[b] = tot;
    dev[b] = d;
    lp[b] = -0.5 * (d + tot);
  }
}

// scal: [kLpScalars][n_chains]; planes LP_S2_MEAN and LP_SS_HAT are inputs (the s2 mean and the SS of theta_mean).
enum : int {
  LP_SS_MIN = 0, LP_SS_MEAN, LP_DEV_MEAN, LP_DEV_VAR, LP_LP_BEST, LP_SS_BEST, LP_S2_BEST, LP_S2_MEAN, LP_SS_HAT,
  LP_D_HAT, LP_P_D, LP_P_V, LP_DIC
};
static_assert(LP_DIC + 1 == kChainlpScalars, "the planes of scal");

__global__ __launch_bounds__(kLpThreads) void k_chainlp_reduce(
    const CellMeta* __restrict__ cells, const double* __restrict__ chain, const double* __restrict__ s2,
    const double* __restrict__ ss, const double* __restrict__ pri, const double* __restrict__ dev,
    const double* __restrict__ lp, const int32_t* __restrict__ cell, int64_t n, int64_t n_chains, int64_t ld, int S,
    double* seg_v, int64_t* seg_r, double* scal, int64_t* __restrict__ best_row, double* __restrict__ theta_best,
    double* theta_mean) {
  __shared__ double sh_mean;
  __shared__ int64_t sh_best;
  const int tid = threadIdx.x;
  const int64_t c = blockIdx.x, nc = n_chains;
  double* sv = seg_v + c * (int64_t)S * kLpSegVals;
  int64_t* sr = seg_r + c * (int64_t)S;
  // pass 1: per segment the sums of ss and dev, the least ss, the first row of the largest lp; row -1: a non-finite
  // ss, pri or dev
  for (int s = tid; s < S; s += kLpThreads) {
    const int64_t r0 = (int64_t)s * kLpSeg;
    const int nr = (int)(n - r0 < kLpSeg ? n - r0 : kLpSeg);
    double a_ss = 0.0, a_dev = 0.0, mn = ss[r0 * nc + c], mx = lp[r0 * nc + c];
    int64_t br = r0;
    bool bad = false;
    for (int i = 0; i < nr; ++i) {
      const int64_t e = (r0 + i) * nc + c;
      const double x = ss[e], p = pri[e], d = dev[e], l = lp[e];
      bad |= !is_finite(x) | !is_finite(p) | !is_finite(d);
      a_ss += x;
      a_dev += d;
      mn = x < mn ? x : mn;
      if (l > mx) {
        mx = l;
        br = r0 + i;
      }
    }
    sv[s * kLpSegVals + 0] = a_ss;
    sv[s * kLpSegVals + 1] = a_dev;
    sv[s * kLpSegVals + 2] = mn;
    sv[s * kLpSegVals + 3] = mx;
    sr[s] = bad ? -1 : br;
  }
  __syncthreads();
  const double dn = (double)n;
  if (tid == 0) {  // the segments in order
    double t_ss = 0.0, t_dev = 0.0, mn = sv[2], mx = sv[3];
    int64_t br = sr[0];
    bool bad = false;
    for (int s = 0; s < S; ++s) {
      t_ss += sv[s * kLpSegVals + 0];
      t_dev += sv[s * kLpSegVals + 1];
      const double m = sv[s * kLpSegVals + 2], x = sv[s * kLpSegVals + 3];
      mn = m < mn ? m : mn;
      bad |= sr[s] < 0;
      if (x > mx) {
        mx = x;
        br = sr[s];
      }
    }
    sh_best = bad ? -1 : br;
    sh_mean = t_dev / dn;
    scal[LP_SS_MIN * nc + c] = mn;
    scal[LP_SS_MEAN * nc + c] = t_ss / dn;
    scal[LP_DEV_MEAN * nc + c] = sh_mean;
  }
  __syncthreads();
  const int64_t best = sh_best;
  const double nan = qnan();
  if (best < 0) {  // the whole workgroup: every reduced output of the chain is NaN
    for (int k = tid; k < kChainlpScalars; k += kLpThreads) scal[k * nc + c] = nan;
    for (int64_t j = tid; j < ld; j += kLpThreads) {
      theta_best[c * ld + j] = nan;
      theta_mean[c * ld + j] = nan;
    }
    if (tid == 0) best_row[c] = -1;
    return;
  }
  // pass 2: the centred squares of dev, in the same segments
  const double dmean = sh_mean;
  for (int s = tid; s < S; s += kLpThreads) {
    const int64_t r0 = (int64_t)s * kLpSeg;
    const int nr = (int)(n - r0 < kLpSeg ? n - r0 : kLpSeg);
    double a = 0.0;
    for (int i = 0; i < nr; ++i) {
      const double d = dev[(r0 + i) * nc + c] - dmean;
      a += d * d;
    }
    sv[s * kLpSegVals + 0] = a;
  }
  __syncthreads();
  const int N = cells[cell[c]].n;
  if (tid == 0) {
    double t = 0.0;
    for (int s = 0; s < S; ++s) t += sv[s * kLpSegVals + 0];
    const double dev_var = t / (double)(n - 1);  // n == 1: 0 / 0
    const int64_t e = best * nc + c;
    const double d_hat = lp_deviance(scal[LP_SS_HAT * nc + c], scal[LP_S2_MEAN * nc + c], (double)(2 * N));
    const double p_d = dmean - d_hat;
    scal[LP_DEV_VAR * nc + c] = dev_var;
    scal[LP_LP_BEST * nc + c] = lp[e];
    scal[LP_SS_BEST * nc + c] = ss[e];
    scal[LP_S2_BEST * nc + c] = s2[e];
    scal[LP_D_HAT * nc + c] = d_hat;
    scal[LP_P_D * nc + c] = p_d;
    scal[LP_P_V * nc + c] = 0.5 * dev_var;
    scal[LP_DIC * nc + c] = dmean + p_d;
    best_row[c] = best;
  }
  const int64_t P = 7 + N;
  const double* row = chain + (best * nc + c) * ld;
  for (int64_t j = tid; j < ld; j += kLpThreads) theta_best[c * ld + j] = j < P ? row[j] : nan;
}

// Segments of a chain of n_rows rows; TCI_ERANGE past the launch grid or the likelihood kernel's.
int lp_sizes(int64_t n_rows, int64_t n_chains, int64_t ld, int64_t* S) {
  if (n_rows < 1 || n_chains < 1 || ld < 1) return TCI_EINVAL;
  if (n_rows > ((int64_t)1 << 30) || n_chains > ((int64_t)1 << 30) || ld > ((int64_t)1 << 24) ||
      (long double)n_rows * (long double)n_chains > 2147483647.0L)
    return TCI_ERANGE;
  *S = (n_rows + kLpSeg - 1) / kLpSeg;
  return TCI_OK;
}

}  // namespace

int chainlp_scratch_bytes(int64_t n_rows, int64_t n_chains, int64_t ld, size_t* bytes) {
  int64_t S;
  const int rc = lp_sizes(n_rows, n_chains, ld, &S);
  if (rc != TCI_OK) return rc;
  *bytes = (size_t)n_chains * (size_t)S * (kLpSegVals * sizeof(double) + sizeof(int64_t));  // below 2^36
  return TCI_OK;
}

int launch_chainlp_ids(const int32_t* cell, int64_t n_rows, int64_t n_chains, int32_t* row_cell, void* stream) {
  int64_t S;
  const int rc = lp_sizes(n_rows, n_chains, 1, &S);
  if (rc != TCI_OK) return rc;
  if (!cell || !row_cell) return TCI_EINVAL;
  const int64_t B = n_rows * n_chains;
  hipLaunchKernelGGL(k_chainlp_ids, dim3((unsigned)((B + kLpThreads - 1) / kLpThreads)), dim3(kLpThreads), 0,
                     (hipStream_t)stream, cell, n_chains, B, row_cell);
  return hipGetLastError() == hipSuccess ? TCI_OK : TCI_EHIP;
}

int launch_chainlp_rows(const KParams& kp, const double* chain, const double* s2, const double* ss, const int32_t* cell,
                        const double* mu, const double* sig, int64_t n_rows, int64_t n_chains, int64_t ld, double* pri,
                        double* dev, double* lp, void* stream) {
  int64_t S;
  const int rc = lp_sizes(n_rows, n_chains, ld, &S);
  if (rc != TCI_OK) return rc;
  if (!chain || !s2 || !ss || !cell || !mu || !sig || !pri || !dev || !lp) return TCI_EINVAL;
  const int64_t B = n_rows * n_chains;
  hipLaunchKernelGGL(k_chainlp_rows, dim3((unsigned)((B + kLpWaves - 1) / kLpWaves)), dim3(kLpThreads), 0,
                     (hipStream_t)stream, kp.cells, chain, s2, ss, cell, mu, sig, n_chains, ld, B, pri, dev, lp);
  return hipGetLastError() == hipSuccess ? TCI_OK : TCI_EHIP;
}

int launch_chainlp_reduce(const KParams& kp, const double* chain, const double* s2, const double* ss, const double* pri,
                          const double* dev, const double* lp, const int32_t* cell, int64_t n_rows, int64_t n_chains,
                          int64_t ld, void* scratch, double* scal, int64_t* best_row, double* theta_best,
                          double* theta_mean, void* stream) {
  int64_t S;
  const int rc = lp_sizes(n_rows, n_chains, ld, &S);
  if (rc != TCI_OK) return rc;
  if (!chain || !s2 || !ss || !pri || !dev || !lp || !cell || !scratch || !scal || !best_row || !theta_best || !theta_mean)
    return TCI_EINVAL;
  double* seg_v = (double*)scratch;
  int64_t* seg_r = (int64_t*)(seg_v + (size_t)n_chains * (size_t)S * kLpSegVals);
  hipLaunchKernelGGL(k_chainlp_reduce, dim3((unsigned)n_chains), dim3(kLpThreads), 0, (hipStream_t)stream, kp.cells, chain,
                     s2, ss, pri, dev, lp, cell, n_rows, n_chains, ld, (int)S, seg_v, seg_r, scal, best_row, theta_best,
                     theta_mean);
  return hipGetLastError() == hipSuccess ? TCI_OK : TCI_EHIP;
}

}  // namespace tci
