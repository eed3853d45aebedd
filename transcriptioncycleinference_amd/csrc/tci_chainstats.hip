// tci_chainstats.hip -- chain convergence diagnostics (mcmcstat's chainstats) reduced on the device.
//
// Per column (one parameter of one chain, or the chain's s2 as one more column) over n diagnostic rows:
// the batch-means Monte-Carlo error (bmstd / sqrt(n)), Sokal's integrated autocorrelation time with its
// adaptive window (iact) and Geweke's z / p with batch-means spectral estimates; formulas in include/tci.h.
//
//   k_cs_moments  one lane per column, two sweeps over the rows: (1) compensated sums of all rows and of
//                 Geweke's two segments, the finite / constant checks; (2) the batch sums of the three
//                 batch-means problems, each centred on its own mean. Writes mcerr, z, p and the column
//                 mean (NaN marks a column k_cs_iact has nothing to do for).
//   k_cs_iact     one workgroup (4 wavefronts) per (chain, 64 columns). Lags go in tiles of 64, 16 per
//                 wavefront; rows in tiles of 32: the centred rows t and t + k0 .. t + k0 + 94 (mod n) of a
//                 tile are staged in LDS once and every lane forms its column's 16 lagged products per row
//                 from there (16 rows x 16 lags of FMAs per 47 LDS reads). After a lag tile wavefront 0
//                 advances Sokal's running sum lag by lag; a column that crossed zero stops, and the
//                 workgroup ends when its last column has.
//
// Every column is summed in row order by one lane, so its statistics depend on the column's values and n
// alone, never on n_chains, ld or the column's position: a shard of a fit gives the whole fit's bits.
#include <hip/hip_runtime.h>

#include <cmath>

#include "tci_chain_dev.h"
#include "tci_csum.h"
#include "tci_fp.h"
#include "tci_internal.h"

namespace tci {

namespace {

// Row `row` of column j <= ld of chain c, addressed from the view's scalars and the lane's j alone.
__device__ __forceinline__ double cs_load(const ChainView& v, int64_t row, int64_t c, int64_t j) {
  return j < v.ld ? v.chain[(row * v.n_chains + c) * v.ld + j] : v.s2[row * v.n_chains + c];
}

// One batch-means problem: nb batches of b rows from the problem's first row, the rest left out;
// q = sum_i (batch mean_i - centre)^2.
struct BatchMeans {
  int b, nb, cnt = 0, done = 0;
  double centre, bs = 0.0, q = 0.0;
  __device__ BatchMeans(int64_t n, double centre_) : centre(centre_) {
    b = (int)(n / 20 > 10 ? n / 20 : 10);
    nb = (int)(n / b);
  }
  __device__ __forceinline__ void add(double x) {
    if (done >= nb) return;
    bs += x - centre;
    if (++cnt == b) {
      const double m = bs / (double)b;
      q += m * m;
      bs = 0.0;
      cnt = 0;
      ++done;
    }
  }
  __device__ double s() const { return sqrt((double)b * q / (double)(nb - 1)); }
};

// out: [5][n_chains * (ld + 1)] = mcerr, tau, geweke z, geweke p, column mean (k_cs_iact's centre).
__global__ __launch_bounds__(kChainCols) void k_cs_moments(ChainView v, int64_t n, int tiles, double* __restrict__ out,
                                                           int32_t* __restrict__ win) {
  const int64_t c = blockIdx.x / tiles;
  const int64_t j = (int64_t)(blockIdx.x % tiles) * kChainCols + threadIdx.x;
  const int64_t ldc = v.ld + 1, plane = v.n_chains * ldc;
  if (j >= ldc) return;
  const int64_t o = c * ldc + j;
  const double nan = qnan();
  if (!chain_live(v, c, j)) {  // padding
    out[o] = out[plane + o] = out[2 * plane + o] = out[3 * plane + o] = out[4 * plane + o] = nan;
    win[o] = -1;
    return;
  }
  const int64_t na = n / 10, nB = n / 2;
  // sweep 1: the means, and whether the column is finite / constant
  CSum all, sa, sb;
  auto load = [&](int64_t r) { return cs_load(v, r, c, j); };
  const double x0 = load(0);
  bool finite = true, same = true;
  col_sweep(n, load, [&](double x, int64_t r) {
    finite &= is_finite(x);
    same &= x == x0;
    all.add(x);
    if (r < na) sa.add(x);
    if (r >= n - nB) sb.add(x);
  });
  if (!finite) {
    out[o] = out[plane + o] = out[2 * plane + o] = out[3 * plane + o] = out[4 * plane + o] = nan;
    win[o] = -1;
    return;
  }
  // a constant column is centred on its value exactly (tau = 0, mcerr = 0, Geweke 0/0)
  const double xbar = same ? x0 : all.total() / (double)n;
  const double ma = same ? x0 : sa.total() / (double)na, mb = same ? x0 : sb.total() / (double)nB;
  // sweep 2: the batch sums, each problem centred on its own mean
  BatchMeans bf(n, xbar), ba(na > 0 ? na : 1, ma), bb(nB > 0 ? nB : 1, mb);
  col_sweep(n, load, [&](double x, int64_t r) {
    bf.add(x);
    if (r < na) ba.add(x);
    if (r >= n - nB) bb.add(x);
  });
  out[o] = n >= 20 ? bf.s() / sqrt((double)n) : nan;
  double z = nan, p = nan;
  if (na >= 20) {  // then nB >= 20 as well
    const double s_a = ba.s(), s_b = bb.s();
    z = (ma - mb) / sqrt(s_a * s_a / (double)na + s_b * s_b / (double)nB);
    p = erfc(fabs(z) / sqrt(2.0));
  }
  out[2 * plane + o] = z;
  out[3 * plane + o] = p;
  out[4 * plane + o] = xbar;
  // tau and the window: k_cs_iact
}

// L: the lags allowed (max_lag, at most n).
__global__ __launch_bounds__(kChainThreads) void k_cs_iact(ChainView v, int64_t n, int64_t L, int tiles,
                                                           double* __restrict__ out, int32_t* __restrict__ win) {
  extern __shared__ __align__(16) double cs_lds[];
  __shared__ int s_live[kChainCols];
  __shared__ int s_any;
  double* A = cs_lds;                        // [kLagRT][64]: centred rows t0 ..
  double* B = cs_lds + kLagRT * kChainCols;  // [kLagBRows][64]: centred rows (t0 + k0 ..) mod n; then c(k) [kLagKT][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t c = blockIdx.x / tiles;
  const int64_t j = (int64_t)(blockIdx.x % tiles) * kChainCols + lane;
  const int64_t ldc = v.ld + 1, plane = v.n_chains * ldc;
  const int64_t o = c * ldc + j;
  // NaN mean: padding or a non-finite column, done before it starts
  const double xb = j < ldc ? out[4 * plane + o] : qnan();
  bool live = xb == xb;
  double S = -1.0 / 3.0, c0 = 0.0, tau = 0.0;
  int32_t w = 0;
  if (wave == 0) lag_publish(s_live, &s_any, lane, live);
  __syncthreads();
  bool any = s_any != 0;
  for (int64_t k0 = 0; any && k0 < L; k0 += kLagKT) {
    double acc[kLagLW];
#pragma unroll
    for (int k = 0; k < kLagLW; ++k) acc[k] = 0.0;
    for (int64_t t0 = 0; t0 < n; t0 += kLagRT)  // the lags are circular: row t's partner is row (t + k) mod n
      lag_tile(A, B, lane, wave, live, t0, t0 + k0,
               [&](int64_t t) { return live && t < n ? cs_load(v, t, c, j) - xb : 0.0; },
               [&](int64_t t) { return live ? cs_load(v, t % n, c, j) - xb : 0.0; }, acc);
    lag_hand(B, lane, wave, live, acc);
    if (wave == 0) {
      if (live) {
        for (int kk = 0; kk < kLagKT; ++kk) {
          const int64_t lag = k0 + kk;
          if (lag >= L) break;
          const double ck = B[kk * kChainCols + lane];
          if (lag == 0) {
            c0 = ck;
            if (c0 == 0.0) {  // a constant column
              tau = 0.0;
              w = 0;
              live = false;
              break;
            }
          }
          S += ck / c0 - 1.0 / 6.0;
          if (S < 0.0) {
            tau = 2.0 * (S + (double)lag / 6.0);
            w = (int32_t)(lag + 1);
            live = false;
            break;
          }
        }
        if (live && k0 + kLagKT >= L) {  // no crossing within the allowed lags
          tau = pinf();
          w = (int32_t)L;
          live = false;
        }
        if (!live) {
          out[plane + o] = tau;
          win[o] = w;
        }
      }
      lag_publish(s_live, &s_any, lane, live);
    }
    __syncthreads();
    live = s_live[lane] != 0;
    any = s_any != 0;
  }
}

}  // namespace

int launch_chainstats(const double* chain, const double* s2, int64_t n_rows, int64_t n_chains, int64_t ld,
                      const int32_t* npar, int64_t max_lag, double* stats, int32_t* win, void* stream) {
  if (!chain || !stats || !win || n_rows < 1 || n_rows > ((int64_t)1 << 30) || n_chains < 1 || ld < 1 || max_lag < 0)
    return TCI_EINVAL;
  const int64_t tiles = (ld + 1 + kChainCols - 1) / kChainCols;
  if (tiles > ((int64_t)1 << 24) || n_chains > ((int64_t)1 << 30) / tiles) return TCI_EINVAL;
  const int64_t L = max_lag == 0 || max_lag > n_rows ? n_rows : max_lag;
  if (ensure_dyn_lds((const void*)k_cs_iact, kLagLds) != TCI_OK) return TCI_EHIP;
  const ChainView v{chain, s2, npar, n_chains, ld};
  const unsigned grid = (unsigned)(n_chains * tiles);
  hipLaunchKernelGGL(k_cs_moments, dim3(grid), dim3(kChainCols), 0, (hipStream_t)stream, v, n_rows, (int)tiles, stats,
                     win);
  if (hipGetLastError() != hipSuccess) return TCI_EHIP;
  hipLaunchKernelGGL(k_cs_iact, dim3(grid), dim3(kChainThreads), kLagLds, (hipStream_t)stream, v, n_rows, L,
                     (int)tiles, stats, win);
  return hipGetLastError() == hipSuccess ? TCI_OK : TCI_EHIP;
}

}  // namespace tci
