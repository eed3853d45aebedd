// tci_chaindens.hip -- marginal posterior density (a Gaussian kernel estimate, mcmcstat's density.m) and
// histogram of every chain column, reduced on the device; the definition is in include/tci.h.
//
// One workgroup (4 wavefronts) takes one segment of a column tile of one chain (tci_chain_dev.h), so a long column
// spreads over many workgroups; the small combine kernels add the segments' partials in segment order.
//
//   k_cd_pass1   per segment: key-order min / max, the non-finite flag and the compensated sum. The wavefronts
//                split the rows (seg_walk) and are combined in order.
//   k_cd_mean    per column: the segments combined; xmin, xmax, the mean and the column's state.
//   k_cd_pass2   per segment: the centred sum of squares.
//   (launch_chainquant gives the quartiles: the project's one quantile definition.)
//   k_cd_params  per column: sd, iqr and the bandwidth.
//   k_cd_dens    per segment: the segment's rows are staged once in LDS (kChainSeg x 64 doubles, 128 KiB), every
//                row's histogram bin next to them (one byte). The four wavefronts split the grid points in groups
//                of four (four independent exp chains per lane); each (column, k) sum runs over the segment's
//                rows in row order. Then the staging area becomes the counter table [B][64] (as k_cq_select's)
//                and the wavefronts add the bins with ds_add_u32: integer counts do not depend on the order.
//   k_cd_out     per output element: the partial sums added in segment order and scaled; NaN / -1 where the
//                definition says so.
// FP64 exp dominates: n_rows x G of them per column; a row costs one LDS read per four of them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "tci_chain_dev.h"
#include "tci_csum.h"
#include "tci_fp.h"
#include "tci_internal.h"
#include "tci_key.h"

namespace tci {

namespace {

constexpr int kCdKU = 4;       // grid points a wavefront evaluates together
constexpr int kCdPar = 4;      // per-column parameters: xmin, xmax, mean, bw
// k_cd_dens stages a whole segment of its 64 columns in LDS, a bin byte next to every row, and reuses the rows'
// area for up to 256 bins of 64 counters
constexpr size_t kCdStage = kChainSeg * kChainCols * sizeof(double);  // 128 KiB
static_assert(kCdStage + kChainSeg * kChainCols * sizeof(uint8_t) <= 160 * 1024, "the stage fits a CU's LDS");
static_assert(256 * kChainCols * sizeof(uint32_t) <= kCdStage, "the counters fit the stage");

// The scratch of one call, carved from one allocation (8-byte items first).
struct CdScratch {
  uint64_t *p_mn, *p_mx;  // [S][ncol] key-order extremes per segment
  double *p_s, *p_c;      // [S][ncol] compensated sum (pass 1); p_s again: centred squares (pass 2)
  double* par;            // [kCdPar][ncol]
  double* q;              // [n_chains][2][ld + 1] quartiles
  double* pd;             // [S][n_chains][G][ld + 1] density partials
  uint32_t* p_bad;        // [S][ncol]
  int32_t* state;         // [ncol]
  uint32_t* pc;           // [S][n_chains][B][ld + 1] count partials
};

__global__ __launch_bounds__(kChainThreads) void k_cd_pass1(ChainView v, int64_t n, int tiles, int S, CdScratch sc) {
  __shared__ uint64_t r_mn[kChainThreads], r_mx[kChainThreads];
  __shared__ double r_s[kChainThreads], r_c[kChainThreads];
  __shared__ uint32_t r_bad[kChainThreads];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const SegWhere w = seg_where(n, tiles, S, lane);
  const int64_t ldc = v.ld + 1, ncol = v.n_chains * ldc;
  const bool live = w.j < ldc && chain_live(v, w.c, w.j);
  const ChainCol col = chain_col(v, w.c, w.j, live);
  uint64_t mn = ~0ull, mx = 0;
  bool bad = false;
  CSum cs;
  seg_walk(col, w, wave, live, 0.0, [&](double x, int i) {
    if (live && i < w.nr) {
      const uint64_t k = to_key(x);
      mn = k < mn ? k : mn;
      mx = k > mx ? k : mx;
      bad |= !is_finite(x);
      cs.add(x);
    }
  });
  r_mn[tid] = mn;
  r_mx[tid] = mx;
  r_s[tid] = cs.s;
  r_c[tid] = cs.c;
  r_bad[tid] = bad ? 1u : 0u;
  __syncthreads();
  if (wave == 0 && w.j < ldc) {  // the wavefronts in order
    uint32_t anybad = r_bad[lane];
    for (int k = 1; k < kChainWaves; ++k) {
      const uint64_t m0 = r_mn[k * kChainCols + lane], m1 = r_mx[k * kChainCols + lane];
      mn = m0 < mn ? m0 : mn;
      mx = m1 > mx ? m1 : mx;
      anybad |= r_bad[k * kChainCols + lane];
      cs.merge(r_s[k * kChainCols + lane], r_c[k * kChainCols + lane]);
    }
    const int64_t o = (int64_t)w.seg * ncol + w.c * ldc + w.j;
    sc.p_mn[o] = mn;
    sc.p_mx[o] = mx;
    sc.p_s[o] = cs.s;
    sc.p_c[o] = cs.c;
    sc.p_bad[o] = anybad;
  }
}

__global__ __launch_bounds__(kChainThreads) void k_cd_mean(ChainView v, int64_t n, int S, CdScratch sc) {
  const int64_t ldc = v.ld + 1, ncol = v.n_chains * ldc;
  const int64_t e = (int64_t)blockIdx.x * kChainThreads + threadIdx.x;
  if (e >= ncol) return;
  const bool live = chain_live(v, e / ldc, e % ldc);
  uint64_t mn = ~0ull, mx = 0;
  uint32_t bad = 0;
  CSum cs;
  for (int s = 0; s < S; ++s) {
    const int64_t o = (int64_t)s * ncol + e;
    const uint64_t m0 = sc.p_mn[o], m1 = sc.p_mx[o];
    mn = m0 < mn ? m0 : mn;
    mx = m1 > mx ? m1 : mx;
    bad |= sc.p_bad[o];
    cs.merge(sc.p_s[o], sc.p_c[o]);
  }
  const bool ok = live && !bad;
  sc.state[e] = !live ? COL_PAD : bad ? COL_BAD : COL_OK;
  sc.par[0 * ncol + e] = ok ? from_key(mn) : 0.0;
  sc.par[1 * ncol + e] = ok ? from_key(mx) : 0.0;
  // a constant column is centred on its value exactly, as tci_chaincov does: sd 0, bw 0
  sc.par[2 * ncol + e] = !ok ? 0.0 : from_key(mn) == from_key(mx) ? from_key(mn) : cs.total() / (double)n;
  sc.par[3 * ncol + e] = 0.0;
}

__global__ __launch_bounds__(kChainThreads) void k_cd_pass2(ChainView v, int64_t n, int tiles, int S, CdScratch sc) {
  __shared__ double r_s[kChainThreads];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const SegWhere w = seg_where(n, tiles, S, lane);
  const int64_t ldc = v.ld + 1, ncol = v.n_chains * ldc;
  const int64_t e = w.c * ldc + w.j;
  const bool ok = w.j < ldc && sc.state[e] == COL_OK;
  const ChainCol col = chain_col(v, w.c, w.j, ok);
  const double mean = ok ? sc.par[2 * ncol + e] : 0.0;
  double ss = 0.0;
  seg_walk(col, w, wave, ok, mean, [&](double x, int) {  // a padded row adds +0.0
    const double d = x - mean;
    ss += d * d;
  });
  r_s[tid] = ss;
  __syncthreads();
  if (wave == 0 && w.j < ldc) {
    for (int k = 1; k < kChainWaves; ++k) ss += r_s[k * kChainCols + lane];
    sc.p_s[(int64_t)w.seg * ncol + e] = ss;
  }
}

__global__ __launch_bounds__(kChainThreads) void k_cd_params(int64_t n_chains, int64_t ld, int64_t n, int S,
                                                             double bw_scale, double npow, CdScratch sc) {
  const int64_t ldc = ld + 1, ncol = n_chains * ldc;
  const int64_t e = (int64_t)blockIdx.x * kChainThreads + threadIdx.x;
  if (e >= ncol) return;
  if (sc.state[e] != COL_OK) return;
  double ss = 0.0;
  for (int s = 0; s < S; ++s) ss += sc.p_s[(int64_t)s * ncol + e];
  const double sd = sqrt(ss / (double)(n - 1));
  const int64_t c = e / ldc, j = e % ldc;
  const double iqr = sc.q[(c * 2 + 1) * ldc + j] - sc.q[(c * 2 + 0) * ldc + j];
  const double s = iqr > 0.0 ? fmin(sd, iqr / 1.34) : sd;
  sc.par[3 * ncol + e] = __dmul_rn(__dmul_rn(__dmul_rn(bw_scale, 1.06), s), npow);
}

__global__ __launch_bounds__(kChainThreads) void k_cd_dens(ChainView v, int64_t n, int tiles, int S, int G, int B,
                                                         CdScratch sc) {
  __shared__ double xs[kChainSeg * kChainCols];    // [row][lane]; afterwards the counter table [bin][lane]
  __shared__ uint8_t bins[kChainSeg * kChainCols];  // [row][lane]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const SegWhere w = seg_where(n, tiles, S, lane);
  const int64_t ldc = v.ld + 1, ncol = v.n_chains * ldc;
  const int64_t e = w.c * ldc + w.j;
  const bool in_out = w.j < ldc;
  const bool ok = in_out && sc.state[e] == COL_OK;
  const ChainCol col = chain_col(v, w.c, w.j, ok);
  const double xmin = ok ? sc.par[0 * ncol + e] : 0.0, xmax = ok ? sc.par[1 * ncol + e] : 0.0;
  const double bw = ok ? sc.par[3 * ncol + e] : 1.0;
  const double r = __dsub_rn(xmax, xmin);
  const double fb = (double)B;
  // stage the segment's rows and their bins
  // seg_walk's loop, written out: this kernel is the reduction's hot spot, and through the helper the compiler
  // schedules it differently (7 % on the whole reduction, profiles/chain_layout/unshared.json)
  for (int i0 = wave * kChainRU; i0 < w.nr; i0 += kChainWaves * kChainRU) {
    double x[kChainRU];
#pragma unroll
    for (int u = 0; u < kChainRU; ++u) x[u] = (ok && i0 + u < w.nr) ? col.ptr[(w.r0 + i0 + u) * col.rs] : xmin;
#pragma unroll
    for (int u = 0; u < kChainRU; ++u)
      if (i0 + u < w.nr) {
        int b = 0;
        if (r > 0.0) {
          b = (int)floor(__dmul_rn(__ddiv_rn(__dsub_rn(x[u], xmin), r), fb));
          b = b > B - 1 ? B - 1 : b < 0 ? 0 : b;
        }
        xs[(i0 + u) * kChainCols + lane] = x[u];
        bins[(i0 + u) * kChainCols + lane] = (uint8_t)b;
      }
  }
  __syncthreads();
  // the grid, as written in the header; the density partials of this segment
  const double w8 = __dmul_rn(0.08, r);
  const double lo = __dsub_rn(xmin, w8), hi = __dadd_rn(xmax, w8);
  const double step = __ddiv_rn(__dsub_rn(hi, lo), (double)(G - 1));
  const double inv = 1.0 / bw;
  for (int kb = wave * kCdKU; kb < G; kb += kChainWaves * kCdKU) {
    double g[kCdKU], a[kCdKU];
#pragma unroll
    for (int u = 0; u < kCdKU; ++u) {
      g[u] = __dadd_rn(lo, __dmul_rn((double)(kb + u), step));
      a[u] = 0.0;
    }
    for (int i = 0; i < w.nr; ++i) {
      const double x = xs[i * kChainCols + lane];
#pragma unroll
      for (int u = 0; u < kCdKU; ++u) {
        const double z = (g[u] - x) * inv;
        a[u] += exp(-0.5 * (z * z));
      }
    }
    if (in_out) {
#pragma unroll
      for (int u = 0; u < kCdKU; ++u)
        if (kb + u < G) sc.pd[(((int64_t)w.seg * v.n_chains + w.c) * G + (kb + u)) * ldc + w.j] = a[u];
    }
  }
  __syncthreads();  // every wavefront is done with the rows
  uint32_t* tab = reinterpret_cast<uint32_t*>(xs);  // B * 64 counters <= 64 KiB
  for (int b = wave; b < B; b += kChainWaves) tab[b * kChainCols + lane] = 0u;
  __syncthreads();
  for (int i = wave; i < w.nr; i += kChainWaves)
    atomicAdd(&tab[(int)bins[i * kChainCols + lane] * kChainCols + lane], 1u);
  __syncthreads();
  if (in_out)
    for (int b = wave; b < B; b += kChainWaves)
      sc.pc[(((int64_t)w.seg * v.n_chains + w.c) * B + b) * ldc + w.j] = tab[b * kChainCols + lane];
}

// out_d: [n_chains][G + 3][ldc] (dens rows, xmin, xmax, bw); out_c: [n_chains][B][ldc]
__global__ __launch_bounds__(kChainThreads) void k_cd_out(int64_t n_chains, int64_t ld, int64_t n, int S, int G, int B,
                                                        CdScratch sc, double* __restrict__ out_d,
                                                        int32_t* __restrict__ out_c) {
  const int64_t ldc = ld + 1, ncol = n_chains * ldc;
  const int64_t rows = G + B + 3;
  const int64_t id = (int64_t)blockIdx.x * kChainThreads + threadIdx.x;
  if (id >= ncol * rows) return;
  const int64_t j = id % ldc, t = (id / ldc) % rows, c = id / ldc / rows;
  const int64_t e = c * ldc + j;
  const bool ok = sc.state[e] == COL_OK;
  const double bw = sc.par[3 * ncol + e];
  if (t < G) {
    double sum = 0.0;
    for (int s = 0; s < S; ++s) sum += sc.pd[(((int64_t)s * n_chains + c) * G + t) * ldc + j];
    const double d = sum / ((double)n * bw) * 0.3989422804014327;  // 1 / sqrt(2 pi)
    out_d[(c * (G + 3) + t) * ldc + j] = ok && bw > 0.0 ? d : qnan();
  } else if (t < G + B) {
    const int64_t b = t - G;
    uint32_t cnt = 0;
    for (int s = 0; s < S; ++s) cnt += sc.pc[(((int64_t)s * n_chains + c) * B + b) * ldc + j];
    out_c[(c * B + b) * ldc + j] = ok ? (int32_t)cnt : -1;
  } else {
    const int64_t k = t - G - B;  // xmin, xmax, bw
    out_d[(c * (G + 3) + G + k) * ldc + j] = !ok ? qnan() : k == 2 ? bw : sc.par[k * ncol + e];
  }
}

// Sizes of one call; false when a launch grid would pass 2^31 - 1 workgroups.
struct CdSizes {
  int64_t S, tiles, ncol, blocks;
  size_t items8, items4;
};
int cd_sizes(int64_t n_rows, int64_t n_chains, int64_t ld, int32_t G, int32_t B, CdSizes* z) {
  if (n_rows < 2 || n_rows > ((int64_t)1 << 30) || n_chains < 1 || n_chains > ((int64_t)1 << 30) || ld < 1 ||
      ld > ((int64_t)1 << 24) || G < 2 || G > 256 || B < 1 || B > 256)
    return TCI_EINVAL;
  z->S = (n_rows + kChainSeg - 1) / kChainSeg;  // <= 2^22
  z->tiles = (ld + 1 + kChainCols - 1) / kChainCols;
  const long double lim = 2147483647.0L;
  const long double ncol = (long double)n_chains * (long double)(ld + 1);
  if (n_chains > ((int64_t)1 << 30) / z->tiles ||  // launch_chainquant's limit
      (long double)n_chains * z->tiles * z->S > lim || ncol * (G + B + 3) / kChainThreads + 1 > lim)
    return TCI_ERANGE;
  const long double i8 = (4.0L * z->S + kCdPar + 2) * ncol + (long double)z->S * ncol * G;
  const long double i4 = ((long double)z->S + 1) * ncol + (long double)z->S * ncol * B;
  if (i8 * 8 + i4 * 4 > (long double)((size_t)1 << 46)) return TCI_ENOMEM;
  z->ncol = n_chains * (ld + 1);  // below 2^46 bytes in all: the integer products cannot overflow
  z->blocks = n_chains * z->tiles * z->S;
  const size_t sn = (size_t)z->S * (size_t)z->ncol;
  z->items8 = 4 * sn + (size_t)(kCdPar + 2) * (size_t)z->ncol + sn * (size_t)G;
  z->items4 = sn + (size_t)z->ncol + sn * (size_t)B;
  return TCI_OK;
}

}  // namespace

int chaindens_scratch_bytes(int64_t n_rows, int64_t n_chains, int64_t ld, int32_t G, int32_t B, size_t* bytes) {
  CdSizes z;
  const int rc = cd_sizes(n_rows, n_chains, ld, G, B, &z);
  if (rc != TCI_OK) return rc;
  *bytes = z.items8 * 8 + z.items4 * 4;
  return TCI_OK;
}

int launch_chaindens(const double* chain, const double* s2, int64_t n_rows, int64_t n_chains, int64_t ld,
                     const int32_t* npar, int32_t G, int32_t B, double bw_scale, double npow, void* scratch,
                     double* out_d, int32_t* out_c, void* stream) {
  if (!chain || !scratch || !out_d || !out_c || !(bw_scale > 0.0) || !(npow > 0.0)) return TCI_EINVAL;
  CdSizes z;
  int rc = cd_sizes(n_rows, n_chains, ld, G, B, &z);
  if (rc != TCI_OK) return rc;
  const size_t sn = (size_t)z.S * (size_t)z.ncol, nc = (size_t)z.ncol;
  CdScratch sc;
  uint64_t* p8 = (uint64_t*)scratch;
  sc.p_mn = p8;
  sc.p_mx = p8 + sn;
  sc.p_s = (double*)(p8 + 2 * sn);
  sc.p_c = (double*)(p8 + 3 * sn);
  sc.par = (double*)(p8 + 4 * sn);
  sc.q = sc.par + kCdPar * nc;
  sc.pd = sc.q + 2 * nc;
  uint32_t* p4 = (uint32_t*)(p8 + z.items8);
  sc.p_bad = p4;
  sc.state = (int32_t*)(p4 + sn);
  sc.pc = p4 + sn + nc;
  const ChainView v{chain, s2, npar, n_chains, ld};
  hipStream_t st = (hipStream_t)stream;
  const dim3 blk(kChainThreads), seg_grid((unsigned)z.blocks);
  const dim3 col_grid((unsigned)((z.ncol + kChainThreads - 1) / kChainThreads));
  const int S = (int)z.S, tiles = (int)z.tiles;
  hipLaunchKernelGGL(k_cd_pass1, seg_grid, blk, 0, st, v, n_rows, tiles, S, sc);
  hipLaunchKernelGGL(k_cd_mean, col_grid, blk, 0, st, v, n_rows, S, sc);
  hipLaunchKernelGGL(k_cd_pass2, seg_grid, blk, 0, st, v, n_rows, tiles, S, sc);
  if (hipGetLastError() != hipSuccess) return TCI_EHIP;
  const double quartiles[2] = {0.25, 0.75};
  rc = launch_chainquant(chain, s2, n_rows, n_chains, ld, npar, quartiles, 2, sc.q, stream);
  if (rc != TCI_OK) return rc;
  hipLaunchKernelGGL(k_cd_params, col_grid, blk, 0, st, n_chains, ld, n_rows, S, bw_scale, npow, sc);
  hipLaunchKernelGGL(k_cd_dens, seg_grid, blk, 0, st, v, n_rows, tiles, S, (int)G, (int)B, sc);
  const int64_t out_items = z.ncol * (int64_t)(G + B + 3);
  hipLaunchKernelGGL(k_cd_out, dim3((unsigned)((out_items + kChainThreads - 1) / kChainThreads)), blk, 0, st, n_chains,
                     ld, n_rows, S, (int)G, (int)B, sc, out_d, out_c);
  return hipGetLastError() == hipSuccess ? TCI_OK : TCI_EHIP;
}

}  // namespace tci
