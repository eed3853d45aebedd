// tci_chainrhat.hip -- Gelman-Rubin's potential scale reduction factor (classic and split R-hat) and the pooled
// posterior mean and standard deviation of every group of chains, reduced on the device; the definition is in
// include/tci.h.
//
// One workgroup (4 wavefronts) takes one segment of a column tile of one chain (tci_chain_dev.h); the per-column
// kernels add the segments' partials in segment order.
//
// Per chain column three sequences are reduced: q = 0 the whole chain, rows [0, n); q = 1 half A, rows [0, h);
// q = 2 half B, rows [n - h, n); h = floor(n / 2).
//
//   k_cr_pass1   per segment: the three compensated sums (a row goes to the sequences it belongs to), the
//                non-finite flag and, per sequence, whether a row differs from the sequence's first. The wavefronts
//                split the rows (seg_walk) and are combined in order.
//   k_cr_mean    per column: the segments combined; the three means and the column's state.
//   k_cr_pass2   per segment: the three centred sums of squares.
//   k_cr_var     per column: the segments combined; the three variances.
//   k_cr_out     per (group, column): the group's sequences in chain order (a CSR list the host built) combined
//                into rhat, rhat_split, pooled_mean and pooled_std; NaN where the definition says so.
// Chains of no group (group[c] < 0) are skipped by every kernel. The row passes are bound by the two reads of
// the chain.
#include <hip/hip_runtime.h>

#include <cmath>

#include "tci_chain_dev.h"
#include "tci_chainrhat_dev.h"
#include "tci_csum.h"
#include "tci_fp.h"
#include "tci_internal.h"

namespace tci {

namespace {

enum : uint32_t { CR_F_BAD = 1u };  // bit 1 + q: sequence q is not constant

// group: [n_chains]; < 0: the chain belongs to no group.
__global__ __launch_bounds__(kChainThreads) void k_cr_pass1(ChainView v, const int32_t* __restrict__ group, int64_t n,
                                                            int64_t h, int tiles, int S, CrScratch sc) {
  __shared__ double r_s[kCrSeq][kChainThreads], r_c[kCrSeq][kChainThreads];
  __shared__ uint32_t r_f[kChainThreads];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const SegWhere w = seg_where(n, tiles, S, lane);
  if (group[w.c] < 0) return;  // the whole workgroup
  const int64_t ldc = v.ld + 1, ncol = v.n_chains * ldc;
  const bool live = w.j < ldc && chain_live(v, w.c, w.j);
  const ChainCol col = chain_col(v, w.c, w.j, live);
  // a sequence's first row: rows 0 (whole, half A) and n - h (half B; h == 0: there is no half)
  const double f0 = live ? col.ptr[0] : 0.0;
  const double fb = live && h > 0 ? col.ptr[(n - h) * col.rs] : 0.0;
  CSum cs[kCrSeq];
  uint32_t fl = 0;
  seg_walk(col, w, wave, live, 0.0, [&](double x, int i) {
    if (live && i < w.nr) {
      const int64_t r = w.r0 + i;
      fl |= !is_finite(x) ? CR_F_BAD : 0u;
      cs[0].add(x);
      fl |= x != f0 ? 2u : 0u;
      if (r < h) {
        cs[1].add(x);
        fl |= x != f0 ? 4u : 0u;
      }
      if (r >= n - h) {
        cs[2].add(x);
        fl |= x != fb ? 8u : 0u;
      }
    }
  });
#pragma unroll
  for (int q = 0; q < kCrSeq; ++q) {
    r_s[q][tid] = cs[q].s;
    r_c[q][tid] = cs[q].c;
  }
  r_f[tid] = fl;
  __syncthreads();
  if (wave == 0 && w.j < ldc) {  // the wavefronts in order
    for (int k = 1; k < kChainWaves; ++k) {
      fl |= r_f[k * kChainCols + lane];
#pragma unroll
      for (int q = 0; q < kCrSeq; ++q) {
        cs[q].merge(r_s[q][k * kChainCols + lane], r_c[q][k * kChainCols + lane]);
      }
    }
    const int64_t e = w.c * ldc + w.j;
#pragma unroll
    for (int q = 0; q < kCrSeq; ++q) {
      sc.p_s[((int64_t)w.seg * kCrSeq + q) * ncol + e] = cs[q].s;
      sc.p_c[((int64_t)w.seg * kCrSeq + q) * ncol + e] = cs[q].c;
    }
    sc.p_f[(int64_t)w.seg * ncol + e] = fl;
  }
}

__global__ __launch_bounds__(kChainThreads) void k_cr_mean(ChainView v, const int32_t* __restrict__ group, int64_t n,
                                                           int64_t h, int S, CrScratch sc) {
  const int64_t ldc = v.ld + 1, ncol = v.n_chains * ldc;
  const int64_t e = (int64_t)blockIdx.x * kChainThreads + threadIdx.x;
  if (e >= ncol) return;
  const int64_t c = e / ldc, j = e % ldc;
  if (group[c] < 0) return;
  const bool live = chain_live(v, c, j);
  if (!live) {
    sc.state[e] = COL_PAD;
    return;
  }
  uint32_t fl = 0;
  CSum cs[kCrSeq];
  for (int s = 0; s < S; ++s) {
    fl |= sc.p_f[(int64_t)s * ncol + e];
#pragma unroll
    for (int q = 0; q < kCrSeq; ++q) {
      cs[q].merge(sc.p_s[((int64_t)s * kCrSeq + q) * ncol + e], sc.p_c[((int64_t)s * kCrSeq + q) * ncol + e]);
    }
  }
  const bool bad = (fl & CR_F_BAD) != 0;
  sc.state[e] = bad ? COL_BAD : COL_OK;
  if (bad) return;
  const ChainCol col = chain_col(v, c, j, true);
  const double f0 = col.ptr[0], fb = h > 0 ? col.ptr[(n - h) * col.rs] : 0.0;
  // a constant sequence is centred on its value exactly, as tci_chaincov does: its variance is exactly 0
  sc.mu[0 * ncol + e] = !(fl & 2u) ? f0 : cs[0].total() / (double)n;
  sc.mu[1 * ncol + e] = h < 1 ? 0.0 : !(fl & 4u) ? f0 : cs[1].total() / (double)h;
  sc.mu[2 * ncol + e] = h < 1 ? 0.0 : !(fl & 8u) ? fb : cs[2].total() / (double)h;
}

__global__ __launch_bounds__(kChainThreads) void k_cr_pass2(ChainView v, const int32_t* __restrict__ group, int64_t n,
                                                            int64_t h, int tiles, int S, CrScratch sc) {
  __shared__ double r_s[kCrSeq][kChainThreads];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const SegWhere w = seg_where(n, tiles, S, lane);
  if (group[w.c] < 0) return;  // the whole workgroup
  const int64_t ldc = v.ld + 1, ncol = v.n_chains * ldc;
  const int64_t e = w.c * ldc + w.j;
  const bool ok = w.j < ldc && sc.state[e] == COL_OK;
  const ChainCol col = chain_col(v, w.c, w.j, ok);
  double mu[kCrSeq], ss[kCrSeq];
#pragma unroll
  for (int q = 0; q < kCrSeq; ++q) {
    mu[q] = ok ? sc.mu[q * ncol + e] : 0.0;
    ss[q] = 0.0;
  }
  seg_walk(col, w, wave, ok, 0.0, [&](double x, int i) {
    if (ok && i < w.nr) {
      const int64_t r = w.r0 + i;
      const double d0 = x - mu[0];
      ss[0] += d0 * d0;
      if (r < h) {
        const double d = x - mu[1];
        ss[1] += d * d;
      }
      if (r >= n - h) {
        const double d = x - mu[2];
        ss[2] += d * d;
      }
    }
  });
#pragma unroll
  for (int q = 0; q < kCrSeq; ++q) r_s[q][tid] = ss[q];
  __syncthreads();
  if (wave == 0 && w.j < ldc) {
#pragma unroll
    for (int q = 0; q < kCrSeq; ++q) {
      for (int k = 1; k < kChainWaves; ++k) ss[q] += r_s[q][k * kChainCols + lane];
      sc.p_s[((int64_t)w.seg * kCrSeq + q) * ncol + e] = ss[q];
    }
  }
}

__global__ __launch_bounds__(kChainThreads) void k_cr_var(ChainView v, const int32_t* __restrict__ group, int64_t n,
                                                          int64_t h, int S, CrScratch sc) {
  const int64_t ldc = v.ld + 1, ncol = v.n_chains * ldc;
  const int64_t e = (int64_t)blockIdx.x * kChainThreads + threadIdx.x;
  if (e >= ncol) return;
  if (group[e / ldc] < 0 || sc.state[e] != COL_OK) return;
#pragma unroll
  for (int q = 0; q < kCrSeq; ++q) {
    double ss = 0.0;
    for (int s = 0; s < S; ++s) ss += sc.p_s[((int64_t)s * kCrSeq + q) * ncol + e];
    const int64_t L = q == 0 ? n : h;
    sc.var[q * ncol + e] = L < 2 ? qnan() : ss / (double)(L - 1);
  }
}

__device__ __forceinline__ double cr_rhat(double sum_v, double dev, int64_t m, int64_t L) {
  if (m < 2 || L < 2) return qnan();
  const double W = sum_v / (double)m;
  const double T = dev / (double)(m - 1);
  return sqrt((double)(L - 1) / (double)L + T / W);
}

// out: [4][n_groups][ldc] = rhat, rhat_split, pooled_mean, pooled_std
__global__ __launch_bounds__(kChainThreads) void k_cr_out(ChainView v, int64_t n, int64_t h, int64_t n_groups,
                                                          const int32_t* __restrict__ g_off,
                                                          const int32_t* __restrict__ g_list, CrScratch sc,
                                                          double* __restrict__ out) {
  const int64_t ldc = v.ld + 1, ncol = v.n_chains * ldc;
  const int64_t id = (int64_t)blockIdx.x * kChainThreads + threadIdx.x;
  if (id >= n_groups * ldc) return;
  const int64_t g = id / ldc, j = id % ldc;
  const int32_t b = g_off[g];
  const int64_t M = g_off[g + 1] - b;
  const int64_t plane = n_groups * ldc;
  double r[4] = {qnan(), qnan(), qnan(), qnan()};
  bool ok = M > 0 && chain_live(v, g_list[b], j);  // the group's chains have one npar (the host checked)
  for (int64_t k = 0; ok && k < M; ++k) ok = sc.state[(int64_t)g_list[b + k] * ldc + j] == COL_OK;
  if (ok) {
    double sv, mb, dv;
    cr_between(CrSeqs{sc.mu, sc.var, g_list + b, ldc, ncol, j, 0, 1}, M, &sv, &mb, &dv);
    r[0] = cr_rhat(sv, dv, M, n);
    r[2] = mb;
    r[3] = sqrt(((double)(n - 1) * sv + (double)n * dv) / ((double)M * (double)n));
    if (h >= 2) {
      double sv2, mb2, dv2;
      cr_between(CrSeqs{sc.mu, sc.var, g_list + b, ldc, ncol, j, 1, 2}, 2 * M, &sv2, &mb2, &dv2);
      r[1] = cr_rhat(sv2, dv2, 2 * M, h);
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) out[t * plane + id] = r[t];
}

// Sizes of one call.
struct CrSizes {
  int64_t S, tiles, ncol, blocks;
  size_t items8, items4;
};
int cr_sizes(int64_t n_rows, int64_t n_chains, int64_t ld, int64_t n_groups, CrSizes* z) {
  if (n_rows < 1 || n_rows > ((int64_t)1 << 30) || n_chains < 1 || n_chains > ((int64_t)1 << 30) || ld < 1 ||
      ld > ((int64_t)1 << 24) || n_groups < 1 || n_groups > n_chains)
    return TCI_EINVAL;
  z->S = (n_rows + kChainSeg - 1) / kChainSeg;  // <= 2^22
  z->tiles = (ld + 1 + kChainCols - 1) / kChainCols;
  const long double lim = 2147483647.0L;
  const long double ncol = (long double)n_chains * (long double)(ld + 1);
  if ((long double)n_chains * z->tiles * z->S > lim || ncol / kChainThreads + 1 > lim) return TCI_ERANGE;
  const long double i8 = (2.0L * kCrSeq * z->S + 2 * kCrSeq) * ncol;
  const long double i4 = ((long double)z->S + 1) * ncol;
  if (i8 * 8 + i4 * 4 > (long double)((size_t)1 << 46)) return TCI_ENOMEM;
  z->ncol = n_chains * (ld + 1);  // below 2^46 bytes in all: the integer products cannot overflow
  z->blocks = n_chains * z->tiles * z->S;
  const size_t sn = (size_t)z->S * (size_t)z->ncol;
  z->items8 = 2 * kCrSeq * sn + 2 * kCrSeq * (size_t)z->ncol;
  z->items4 = sn + (size_t)z->ncol;
  return TCI_OK;
}

// The scratch's arrays.
CrScratch cr_carve(void* scratch, const CrSizes& z) {
  const size_t sn = (size_t)z.S * (size_t)z.ncol, nc = (size_t)z.ncol;
  CrScratch sc;
  double* p8 = (double*)scratch;
  sc.p_s = p8;
  sc.p_c = p8 + kCrSeq * sn;
  sc.mu = p8 + 2 * kCrSeq * sn;
  sc.var = sc.mu + kCrSeq * nc;
  uint32_t* p4 = (uint32_t*)(p8 + z.items8);
  sc.p_f = p4;
  sc.state = (int32_t*)(p4 + sn);
  return sc;
}

}  // namespace

int chainrhat_scratch_moments(void* scratch, int64_t n_rows, int64_t n_chains, int64_t ld, int64_t n_groups,
                              const double** mu, const double** var, const int32_t** state) {
  CrSizes z;
  const int rc = cr_sizes(n_rows, n_chains, ld, n_groups, &z);
  if (rc != TCI_OK) return rc;
  const CrScratch sc = cr_carve(scratch, z);
  *mu = sc.mu;
  *var = sc.var;
  *state = sc.state;
  return TCI_OK;
}

int chainrhat_scratch_bytes(int64_t n_rows, int64_t n_chains, int64_t ld, int64_t n_groups, size_t* bytes) {
  CrSizes z;
  const int rc = cr_sizes(n_rows, n_chains, ld, n_groups, &z);
  if (rc != TCI_OK) return rc;
  *bytes = z.items8 * 8 + z.items4 * 4;
  return TCI_OK;
}

int launch_chainrhat(const double* chain, const double* s2, int64_t n_rows, int64_t n_chains, int64_t ld,
                     const int32_t* npar, const int32_t* group, int64_t n_groups, const int32_t* g_off,
                     const int32_t* g_list, void* scratch, double* out, void* stream) {
  if (!chain || !group || !g_off || !g_list || !scratch || !out) return TCI_EINVAL;
  CrSizes z;
  const int rc = cr_sizes(n_rows, n_chains, ld, n_groups, &z);
  if (rc != TCI_OK) return rc;
  const CrScratch sc = cr_carve(scratch, z);
  const ChainView v{chain, s2, npar, n_chains, ld};
  const int64_t h = n_rows / 2;
  hipStream_t st = (hipStream_t)stream;
  const dim3 blk(kChainThreads), seg_grid((unsigned)z.blocks);
  const dim3 col_grid((unsigned)((z.ncol + kChainThreads - 1) / kChainThreads));
  const int S = (int)z.S, tiles = (int)z.tiles;
  hipLaunchKernelGGL(k_cr_pass1, seg_grid, blk, 0, st, v, group, n_rows, h, tiles, S, sc);
  hipLaunchKernelGGL(k_cr_mean, col_grid, blk, 0, st, v, group, n_rows, h, S, sc);
  hipLaunchKernelGGL(k_cr_pass2, seg_grid, blk, 0, st, v, group, n_rows, h, tiles, S, sc);
  hipLaunchKernelGGL(k_cr_var, col_grid, blk, 0, st, v, group, n_rows, h, S, sc);
  const int64_t out_items = n_groups * (ld + 1);
  hipLaunchKernelGGL(k_cr_out, dim3((unsigned)((out_items + kChainThreads - 1) / kChainThreads)), blk, 0, st, v, n_rows,
                     h, n_groups, g_off, g_list, sc, out);
  return hipGetLastError() == hipSuccess ? TCI_OK : TCI_EHIP;
}

}  // namespace tci
