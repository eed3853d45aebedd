// tci_chaincov.hip -- posterior mean, covariance and correlation of every chain (MATLAB's mean / cov / corrcoef
// of the chain matrix), reduced on the device; formulas in include/tci.h.
//
//   k_cc_mean  one lane per column, as k_cs_moments: the compensated sum of the column in row order, the
//              finite / constant checks. NaN marks padding and a column holding a non-finite value.
//   k_cc_cov   one workgroup (4 wavefronts) per (chain, tile row I). Wavefront w owns the tiles J = I + w,
//              I + w + 4, .. (J >= I only), kCcJ of them per sweep over the rows. Per four rows lane 16 g + j
//              loads row t + g of column 16 I + j once (the A operand), and of column 16 J + j per tile (the B
//              operand), both centred on their means, and every tile takes one v_mfma_f64_16x16x4. Rows are
//              read straight from global memory (a 16-lane group reads 128 contiguous bytes), 16 rows of loads
//              in flight. The upper triangle is written and mirrored, so cov is symmetric bit for bit.
//   k_cc_corr  elementwise from cov.
//
// Rows are never split: one wavefront sums a tile over all rows in order, so an element's bits depend on its two
// columns, their indices and n alone, never on n_chains, on the chain's position or on ld.
#include <hip/hip_runtime.h>

#include <cmath>

#include "tci_chain_dev.h"
#include "tci_csum.h"
#include "tci_fp.h"
#include "tci_internal.h"
#include "tci_tile16.h"

namespace tci {

namespace {

constexpr int kCcJ = 4;    // tiles a wavefront accumulates per sweep over the rows (4 accumulator registers each)
constexpr int kCcRU = 4;   // groups of four rows whose loads are issued together

// The view's s2 is null: the covariance is of the parameters. c0 is the first chain of a launch: mean is indexed by
// chain, cov / corr by chain - c0.
__global__ __launch_bounds__(kChainCols) void k_cc_mean(ChainView v, int64_t c0, int64_t n, int tiles,
                                                        double* __restrict__ mean) {
  const int64_t c = c0 + blockIdx.x / tiles;
  const int64_t j = (int64_t)(blockIdx.x % tiles) * kChainCols + threadIdx.x;
  if (j >= v.ld) return;
  double* out = mean + c * v.ld + j;
  if (!chain_live(v, c, j)) {  // padding
    *out = qnan();
    return;
  }
  const ChainCol col = chain_col(v, c, j, true);
  CSum all;
  const double x0 = col.ptr[0];
  bool finite = true, same = true;
  col_sweep(n, [&](int64_t r) { return col.ptr[r * col.rs]; }, [&](double x, int64_t) {
    finite &= is_finite(x);
    same &= x == x0;
    all.add(x);
  });
  // a constant column is centred on its value exactly (cov 0, corr 0/0)
  *out = !finite ? qnan() : same ? x0 : all.total() / (double)n;
}

// cov: [chains of the launch][ld][ld]. NT = ceil(ld / 16).
__global__ __launch_bounds__(256) void k_cc_cov(ChainView v, int64_t c0, int64_t n, int NT,
                                                const double* __restrict__ mean, double* __restrict__ cov) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, jl = lane & 15;
  const int64_t cl = blockIdx.x / NT, c = c0 + cl, ld = v.ld;
  const int I = (int)(blockIdx.x % NT);
  const int64_t P = chain_npar(v, c);
  const int NTP = (int)((P + 15) / 16);  // tiles holding a real column
  const double* mc = mean + c * ld;
  double* covc = cov + cl * ld * ld;
  const double nan = qnan();
  if (I < NTP) {
    const int64_t rs = v.n_chains * ld;
    const double* base = v.chain + c * ld;
    // the A operand's column: padding and non-finite columns enter as zeros and are masked when written
    const int64_t ia = 16 * (int64_t)I + jl;
    const double ma = ia < P ? mc[ia] : nan;
    const bool oka = ma == ma;
    const double* pa = base + (oka ? ia : 0);
    for (int J0 = I + wave; J0 < NTP; J0 += 4 * kCcJ) {
      int nu = 0;
      double mb[kCcJ];
      bool okb[kCcJ];
      const double* pb[kCcJ];
      f64x4 acc[kCcJ];
#pragma unroll
      for (int u = 0; u < kCcJ; ++u) {
        const int J = J0 + 4 * u;
        if (J < NTP) nu = u + 1;
        const int64_t jb = 16 * (int64_t)J + jl;
        mb[u] = (J < NTP && jb < P) ? mc[jb] : nan;
        okb[u] = mb[u] == mb[u];
        pb[u] = base + (okb[u] ? jb : 0);
        acc[u] = f64x4{0.0, 0.0, 0.0, 0.0};
      }
      int64_t t = 0;
      // 4 * kCcRU whole rows: every load is issued before the first MFMA needs one
      for (; t + 4 * kCcRU <= n; t += 4 * kCcRU) {
        double a[kCcRU], b[kCcJ][kCcRU];
#pragma unroll
        for (int k = 0; k < kCcRU; ++k) {
          const int64_t ro = (t + 4 * k + g) * rs;
          a[k] = oka ? pa[ro] - ma : 0.0;
#pragma unroll
          for (int u = 0; u < kCcJ; ++u) b[u][k] = (u < nu && okb[u]) ? pb[u][ro] - mb[u] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < kCcRU; ++k)
#pragma unroll
          for (int u = 0; u < kCcJ; ++u)
            if (u < nu) acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[k], b[u][k], acc[u], 0, 0, 0);
      }
      // the rest, four rows at a time; rows past n enter as zeros
      for (; t < n; t += 4) {
        const bool in = t + g < n;
        const int64_t ro = (in ? t + g : 0) * rs;
        const double a = (in && oka) ? pa[ro] - ma : 0.0;
#pragma unroll
        for (int u = 0; u < kCcJ; ++u) {
          if (u >= nu) continue;
          const double b = (in && okb[u]) ? pb[u][ro] - mb[u] : 0.0;
          acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[u], 0, 0, 0);
        }
      }
      // lane 16 g + j holds rows 4 q + g of column j
      const double nm1 = (double)(n - 1);
#pragma unroll
      for (int u = 0; u < kCcJ; ++u) {
        if (u >= nu) continue;
        const int J = J0 + 4 * u;
        const int64_t jj = 16 * (int64_t)J + jl;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int64_t i = 16 * (int64_t)I + 4 * q + g;
          if (i >= ld || jj >= ld || (I == J && i > jj)) continue;
          const double mi = i < P ? mc[i] : nan;
          const double val = (mi == mi && okb[u]) ? acc[u][q] / nm1 : nan;
          covc[i * ld + jj] = val;
          if (i != jj) covc[jj * ld + i] = val;
        }
      }
    }
  }
  // the padding right of the real tiles (or the whole tile row when it is padding), and its mirror
  const int64_t j0 = 16 * (int64_t)(I < NTP ? NTP : I);
  const int64_t w = ld - j0;
  for (int64_t e = tid; e < 16 * w; e += 256) {
    const int64_t i = 16 * (int64_t)I + e / w, jj = j0 + e % w;
    if (i >= ld) break;
    covc[i * ld + jj] = nan;
    covc[jj * ld + i] = nan;
  }
}

// One workgroup per (chain, row i).
__global__ __launch_bounds__(128) void k_cc_corr(ChainView v, int64_t c0, const double* __restrict__ cov,
                                                 double* __restrict__ corr) {
  const int64_t ld = v.ld, cl = blockIdx.x / ld, i = blockIdx.x % ld;
  const int64_t P = chain_npar(v, c0 + cl);
  const double* covc = cov + cl * ld * ld;
  double* out = corr + cl * ld * ld + i * ld;
  const double nan = qnan();
  const double cii = covc[i * ld + i];
  const double si = sqrt(cii);
  for (int64_t j = threadIdx.x; j < ld; j += 128) {
    double r = nan;
    if (i < P && j < P) {
      if (i == j) {
        r = (cii > 0.0 && is_finite(cii)) ? 1.0 : nan;
      } else {
        r = covc[i * ld + j] / (si * sqrt(covc[j * ld + j]));
        r = r > 1.0 ? 1.0 : r < -1.0 ? -1.0 : r;  // keeps NaN
      }
    }
    out[j] = r;
  }
}

}  // namespace

int launch_chaincov(const double* chain, int64_t n_rows, int64_t n_chains, int64_t ld, const int32_t* npar, int64_t c0,
                    int64_t nc, double* mean, double* cov, double* corr, void* stream) {
  if (!chain || !mean || !cov || !corr || n_rows < 2 || n_rows > ((int64_t)1 << 30) || n_chains < 1 || ld < 1 ||
      ld > ((int64_t)1 << 24) || c0 < 0 || nc < 1 || c0 + nc > n_chains)
    return TCI_EINVAL;
  if (nc > chaincov_max_chains(ld)) return TCI_EINVAL;
  const int64_t tiles = (ld + kChainCols - 1) / kChainCols, NT = (ld + 15) / 16;
  const ChainView v{chain, nullptr, npar, n_chains, ld};
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_cc_mean, dim3((unsigned)(nc * tiles)), dim3(kChainCols), 0, s, v, c0, n_rows, (int)tiles,
                     mean);
  if (hipGetLastError() != hipSuccess) return TCI_EHIP;
  hipLaunchKernelGGL(k_cc_cov, dim3((unsigned)(nc * NT)), dim3(256), 0, s, v, c0, n_rows, (int)NT, mean, cov);
  if (hipGetLastError() != hipSuccess) return TCI_EHIP;
  hipLaunchKernelGGL(k_cc_corr, dim3((unsigned)(nc * ld)), dim3(128), 0, s, v, c0, cov, corr);
  return hipGetLastError() == hipSuccess ? TCI_OK : TCI_EHIP;
}

int launch_chain_mean(const double* chain, int64_t n_rows, int64_t n_chains, int64_t ld, const int32_t* npar,
                      double* mean, void* stream) {
  if (!chain || !mean || n_rows < 1 || n_rows > ((int64_t)1 << 30) || n_chains < 1 || ld < 1 || ld > ((int64_t)1 << 24))
    return TCI_EINVAL;
  const int64_t tiles = (ld + kChainCols - 1) / kChainCols;
  if (n_chains * tiles > 2147483647) return TCI_EINVAL;
  const ChainView v{chain, nullptr, npar, n_chains, ld};
  hipLaunchKernelGGL(k_cc_mean, dim3((unsigned)(n_chains * tiles)), dim3(kChainCols), 0, (hipStream_t)stream, v,
                     (int64_t)0, n_rows, (int)tiles, mean);
  return hipGetLastError() == hipSuccess ? TCI_OK : TCI_EHIP;
}

int64_t chaincov_max_chains(int64_t ld) { return ((int64_t)1 << 30) / (ld > 1 ? ld : 1); }

}  // namespace tci
