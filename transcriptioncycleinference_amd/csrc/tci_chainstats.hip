// tci_chainstats.hip -- chain convergence diagnostics (mcmcstat's chainstats) reduced on the device.
//
// Per column (one parameter of one chain, or the chain's s2 as one more column) over n diagnostic rows:
// the batch-means Monte-Carlo error (bmstd / sqrt(n)), Sokal's integrated autocorrelation time with its
// adaptive window (iact) and Geweke's z / p with batch-means spectral estimates; formulas in include/tci.h.
//
// The chain lies as [rows][n_chains][ld]: contiguous along the parameter, so the 64 lanes of a wavefront
// take 64 consecutive parameters of one chain and every row read is one 512 B segment.
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

#include "tci_csum.h"
#include "tci_internal.h"

namespace tci {

namespace {

constexpr int kCsCols = 64;                    // columns per workgroup: one per lane
constexpr int kCsRT = 32;                      // rows per LDS tile
constexpr int kCsKT = 64;                      // lags per tile
constexpr int kCsLW = 16;                      // lags per wavefront (kCsKT / 4)
constexpr int kCsBRows = kCsRT + kCsKT - 1;    // shifted rows a tile needs
constexpr size_t kCsLds = (size_t)(kCsRT + kCsBRows) * kCsCols * sizeof(double);  // 65,024 B: two workgroups per CU

struct CsView {
  const double* chain;  // [rows][n_chains][ld]
  const double* s2;     // [rows][n_chains] or null
  int64_t n_chains, ld;
};

// Column j < ld: a parameter; j == ld: the chain's s2.
__device__ __forceinline__ double cs_load(const CsView& v, int64_t row, int64_t c, int64_t j) {
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

__device__ __forceinline__ double cs_nan() { return __longlong_as_double(0x7FF8000000000000ll); }

// out: [5][n_chains * (ld + 1)] = mcerr, tau, geweke z, geweke p, column mean (k_cs_iact's centre).
__global__ __launch_bounds__(kCsCols) void k_cs_moments(CsView v, const int32_t* __restrict__ npar, int64_t n,
                                                        int tiles, double* __restrict__ out,
                                                        int32_t* __restrict__ win) {
  const int64_t c = blockIdx.x / tiles;
  const int64_t j = (int64_t)(blockIdx.x % tiles) * kCsCols + threadIdx.x;
  const int64_t ldc = v.ld + 1, plane = v.n_chains * ldc;
  if (j >= ldc) return;
  const int64_t o = c * ldc + j;
  const double nan = cs_nan();
  const bool is_col = j < v.ld ? j < (npar ? (int64_t)npar[c] : v.ld) : v.s2 != nullptr;
  if (!is_col) {  // padding
    out[o] = out[plane + o] = out[2 * plane + o] = out[3 * plane + o] = out[4 * plane + o] = nan;
    win[o] = -1;
    return;
  }
  const int64_t na = n / 10, nB = n / 2;
  // sweep 1: the means, and whether the column is finite / constant
  CSum all, sa, sb;
  const double x0 = cs_load(v, 0, c, j);
  bool finite = true, same = true;
  auto first = [&](double x, int64_t r) {
    finite &= (x - x) == 0.0;
    same &= x == x0;
    all.add(x);
    if (r < na) sa.add(x);
    if (r >= n - nB) sb.add(x);
  };
  int64_t r = 0;
  for (; r + 8 <= n; r += 8) {
    double x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = cs_load(v, r + u, c, j);
#pragma unroll
    for (int u = 0; u < 8; ++u) first(x[u], r + u);
  }
  for (; r < n; ++r) first(cs_load(v, r, c, j), r);
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
  auto second = [&](double x, int64_t rr) {
    bf.add(x);
    if (rr < na) ba.add(x);
    if (rr >= n - nB) bb.add(x);
  };
  for (r = 0; r + 8 <= n; r += 8) {
    double x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = cs_load(v, r + u, c, j);
#pragma unroll
    for (int u = 0; u < 8; ++u) second(x[u], r + u);
  }
  for (; r < n; ++r) second(cs_load(v, r, c, j), r);
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
__global__ __launch_bounds__(256) void k_cs_iact(CsView v, int64_t n, int64_t L, int tiles, double* __restrict__ out,
                                                 int32_t* __restrict__ win) {
  extern __shared__ __align__(16) double cs_lds[];
  __shared__ int s_live[kCsCols];
  __shared__ int s_any;
  double* A = cs_lds;                    // [kCsRT][64]: centred rows t0 ..
  double* B = cs_lds + kCsRT * kCsCols;  // [kCsBRows][64]: centred rows (t0 + k0 ..) mod n; then c(k) [kCsKT][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t c = blockIdx.x / tiles;
  const int64_t j = (int64_t)(blockIdx.x % tiles) * kCsCols + lane;
  const int64_t ldc = v.ld + 1, plane = v.n_chains * ldc;
  const int64_t o = c * ldc + j;
  // NaN mean: padding or a non-finite column, done before it starts
  const double xb = j < ldc ? out[4 * plane + o] : cs_nan();
  bool live = xb == xb;
  double S = -1.0 / 3.0, c0 = 0.0, tau = 0.0;
  int32_t w = 0;
  if (wave == 0) {
    s_live[lane] = live;
    const bool any = __ballot(live) != 0;
    if (lane == 0) s_any = any;
  }
  __syncthreads();
  bool any = s_any != 0;
  for (int64_t k0 = 0; any && k0 < L; k0 += kCsKT) {
    double acc[kCsLW];
#pragma unroll
    for (int k = 0; k < kCsLW; ++k) acc[k] = 0.0;
    for (int64_t t0 = 0; t0 < n; t0 += kCsRT) {
      __syncthreads();  // the previous tile (or the previous lag tile's c(k)) has been read
      for (int i = wave; i < kCsRT; i += 4) {
        const int64_t t = t0 + i;
        A[i * kCsCols + lane] = live && t < n ? cs_load(v, t, c, j) - xb : 0.0;
      }
      for (int r = wave; r < kCsBRows; r += 4)
        B[r * kCsCols + lane] = live ? cs_load(v, (t0 + k0 + r) % n, c, j) - xb : 0.0;
      __syncthreads();
      if (live) {
#pragma unroll
        for (int ib = 0; ib < kCsRT; ib += kCsLW) {
          double a[kCsLW], b[2 * kCsLW - 1];
#pragma unroll
          for (int u = 0; u < kCsLW; ++u) a[u] = A[(ib + u) * kCsCols + lane];
#pragma unroll
          for (int u = 0; u < 2 * kCsLW - 1; ++u) b[u] = B[(ib + kCsLW * wave + u) * kCsCols + lane];
#pragma unroll
          for (int i = 0; i < kCsLW; ++i)  // rows in order: lag k sums y[t] * y[t + k] over increasing t
#pragma unroll
            for (int k = 0; k < kCsLW; ++k) acc[k] = fma(a[i], b[i + k], acc[k]);
        }
      }
    }
    __syncthreads();
    if (live)
#pragma unroll
      for (int k = 0; k < kCsLW; ++k) B[(kCsLW * wave + k) * kCsCols + lane] = acc[k];
    __syncthreads();
    if (wave == 0) {
      if (live) {
        for (int kk = 0; kk < kCsKT; ++kk) {
          const int64_t lag = k0 + kk;
          if (lag >= L) break;
          const double ck = B[kk * kCsCols + lane];
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
        if (live && k0 + kCsKT >= L) {  // no crossing within the allowed lags
          tau = __longlong_as_double(0x7FF0000000000000ll);
          w = (int32_t)L;
          live = false;
        }
        if (!live) {
          out[plane + o] = tau;
          win[o] = w;
        }
      }
      s_live[lane] = live;
      const bool a2 = __ballot(live) != 0;
      if (lane == 0) s_any = a2;
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
  const int64_t tiles = (ld + 1 + kCsCols - 1) / kCsCols;
  if (tiles > ((int64_t)1 << 24) || n_chains > ((int64_t)1 << 30) / tiles) return TCI_EINVAL;
  const int64_t L = max_lag == 0 || max_lag > n_rows ? n_rows : max_lag;
  if (ensure_dyn_lds((const void*)k_cs_iact, kCsLds) != TCI_OK) return TCI_EHIP;
  const CsView v{chain, s2, n_chains, ld};
  const unsigned grid = (unsigned)(n_chains * tiles);
  hipLaunchKernelGGL(k_cs_moments, dim3(grid), dim3(kCsCols), 0, (hipStream_t)stream, v, npar, n_rows, (int)tiles,
                     stats, win);
  if (hipGetLastError() != hipSuccess) return TCI_EHIP;
  hipLaunchKernelGGL(k_cs_iact, dim3(grid), dim3(256), kCsLds, (hipStream_t)stream, v, n_rows, L, (int)tiles, stats,
                     win);
  return hipGetLastError() == hipSuccess ? TCI_OK : TCI_EHIP;
}

}  // namespace tci
