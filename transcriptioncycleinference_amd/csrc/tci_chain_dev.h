// tci_chain_dev.h -- what the chain reductions (tci_chain*.hip) share on the device: the chain's layout, which of
// its columns are real, the tile and segment a workgroup takes, and the three row walks.
//
// The chain lies as [rows][n_chains][ld], contiguous along the parameter, and its s2 as [rows][n_chains]: column
// j < ld of chain c is a parameter, column ld the chain's s2, so a chain has ldc = ld + 1 columns. A chain with
// npar[c] < ld parameters is padded up to ld; without s2 column ld is padding too. 64 consecutive columns of one
// chain make a column tile, lane l of every wavefront taking column 64 t + l, so a row read is one 512 B segment.
// Every reduction sums a column's rows in an order that follows from n_rows alone, so an output's bits depend on
// the column's values and n_rows, never on n_chains, ld, the column's position or how many workgroups ran.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tci {

namespace {

struct ChainView {
  const double* chain;  // [rows][n_chains][ld]
  const double* s2;     // [rows][n_chains] or null
  const int32_t* npar;  // [n_chains] or null
  int64_t n_chains, ld;
};

__device__ __forceinline__ int64_t chain_npar(const ChainView& v, int64_t c) {
  return v.npar ? (int64_t)v.npar[c] : v.ld;
}

// Whether column j of chain c is a real column, not padding.
__device__ __forceinline__ bool chain_live(const ChainView& v, int64_t c, int64_t j) {
  return j < v.ld ? j < chain_npar(v, c) : (j == v.ld && v.s2 != nullptr);
}

// Row 0 of column j of chain c and the stride of a row; a column the caller does not mean to read (!live) gets no
// address. Every load is guarded by its caller as well: the null is there because without it the compiler orders
// k_cq_select and the segment passes differently ("What the chain reductions share").
struct ChainCol {
  const double* ptr;
  int64_t rs;
};
__device__ __forceinline__ ChainCol chain_col(const ChainView& v, int64_t c, int64_t j, bool live) {
  return {!live ? nullptr : j < v.ld ? v.chain + c * v.ld + j : v.s2 + c, j < v.ld ? v.n_chains * v.ld : v.n_chains};
}

// A column's state in a reduction's scratch.
enum : int32_t { COL_PAD = 0, COL_OK = 1, COL_BAD = 2 };  // padding; finite; holds a non-finite value

constexpr int kChainCols = 64;   // columns per workgroup: one per lane
constexpr int kChainWaves = 4;   // wavefronts per workgroup
constexpr int kChainRU = 8;      // rows a lane loads together
constexpr int kChainSeg = 256;   // rows per segment
constexpr int kChainThreads = kChainCols * kChainWaves;
static_assert(kChainSeg % (kChainWaves * kChainRU) == 0, "a whole segment is whole row blocks for every wavefront");

// The workgroup's chain, column and segment: blockIdx.x = (chain * tiles + tile) * S + segment. The segment count
// S = ceil(n / kChainSeg) and the boundaries follow from n alone; partials are stored per segment and added in
// segment order.
struct SegWhere {
  int64_t c, j, r0;
  int nr, seg;
};
__device__ __forceinline__ SegWhere seg_where(int64_t n, int tiles, int S, int lane) {
  SegWhere w;
  const int64_t ct = (int64_t)blockIdx.x / S;
  w.seg = (int)((int64_t)blockIdx.x % S);
  w.c = ct / tiles;
  w.j = (ct % tiles) * kChainCols + lane;
  w.r0 = (int64_t)w.seg * kChainSeg;
  w.nr = (int)(n - w.r0 < kChainSeg ? n - w.r0 : kChainSeg);
  return w;
}

// A wavefront's share of a segment: the blocks of kChainRU rows wave, wave + 4, .., a block's loads issued together,
// then body(x, i) for the rows r0 + i of the block in order. A lane with !on and the rows past the segment load
// nothing and hand pad to body, which knows which of them it wants.
template <class F>
__device__ __forceinline__ void seg_walk(const ChainCol& col, const SegWhere& w, int wave, bool on, double pad,
                                         F&& body) {
  for (int i0 = wave * kChainRU; i0 < w.nr; i0 += kChainWaves * kChainRU) {
    double x[kChainRU];
#pragma unroll
    for (int u = 0; u < kChainRU; ++u) x[u] = (on && i0 + u < w.nr) ? col.ptr[(w.r0 + i0 + u) * col.rs] : pad;
#pragma unroll
    for (int u = 0; u < kChainRU; ++u) body(x[u], i0 + u);
  }
}

// One lane's sweep over all n rows of its column in row order: kChainRU rows loaded together, then a scalar tail;
// x = load(r), then body(x, r) per row. (The caller loads: k_cs_moments addresses a row from scalars, which a
// per-lane pointer and stride would cost it an occupancy step for.)
template <class L, class F>
__device__ __forceinline__ void col_sweep(int64_t n, L&& load, F&& body) {
  int64_t r = 0;
  for (; r + kChainRU <= n; r += kChainRU) {
    double x[kChainRU];
#pragma unroll
    for (int u = 0; u < kChainRU; ++u) x[u] = load(r + u);
#pragma unroll
    for (int u = 0; u < kChainRU; ++u) body(x[u], r + u);
  }
  for (; r < n; ++r) body(load(r), r);
}

// The lagged-product tile of k_cs_iact and k_ce_lags: a workgroup of kChainWaves wavefronts holds 64 columns, lags
// go in tiles of kLagKT (kLagLW per wavefront), rows in tiles of kLagRT.
constexpr int kLagRT = 32;                       // rows per LDS tile
constexpr int kLagKT = 64;                       // lags per tile
constexpr int kLagLW = kLagKT / kChainWaves;     // lags per wavefront
constexpr int kLagBRows = kLagRT + kLagKT - 1;   // shifted rows a tile needs
// 65,024 B: two workgroups per CU
constexpr size_t kLagLds = (size_t)(kLagRT + kLagBRows) * kChainCols * sizeof(double);
static_assert(kLagRT % kLagLW == 0, "a row tile is whole 16 x 16 blocks");

// One row tile of one lag tile. A [kLagRT][64] takes ya(t0 ..) and B [kLagBRows][64] takes yb(tb0 ..), the centred
// rows of the lane's column; the caller's ya / yb give 0, and load nothing, where the sequence has no such row and
// in a lane that is not live. Then every live lane adds its column's kLagLW lagged products per row to acc, rows in
// order: lag k sums y[t] * y[t + k] over increasing t with one FMA per product.
template <class FA, class FB>
__device__ __forceinline__ void lag_tile(double* A, double* B, int lane, int wave, bool live, int64_t t0, int64_t tb0,
                                         FA&& ya, FB&& yb, double (&acc)[kLagLW]) {
  __syncthreads();  // the previous tile (or the previous lag tile's sums) has been read
  for (int i = wave; i < kLagRT; i += kChainWaves) A[i * kChainCols + lane] = ya(t0 + i);
  for (int r = wave; r < kLagBRows; r += kChainWaves) B[r * kChainCols + lane] = yb(tb0 + r);
  __syncthreads();
  if (live) {
#pragma unroll
    for (int ib = 0; ib < kLagRT; ib += kLagLW) {
      double a[kLagLW], b[2 * kLagLW - 1];
#pragma unroll
      for (int u = 0; u < kLagLW; ++u) a[u] = A[(ib + u) * kChainCols + lane];
#pragma unroll
      for (int u = 0; u < 2 * kLagLW - 1; ++u) b[u] = B[(ib + kLagLW * wave + u) * kChainCols + lane];
#pragma unroll
      for (int i = 0; i < kLagLW; ++i)
#pragma unroll
        for (int k = 0; k < kLagLW; ++k) acc[k] = fma(a[i], b[i + k], acc[k]);
    }
  }
}

// The lag tile's sums of all four wavefronts laid into B as [kLagKT][64] for wavefront 0 to walk.
__device__ __forceinline__ void lag_hand(double* B, int lane, int wave, bool live, const double (&sum)[kLagLW]) {
  __syncthreads();
  if (live)
#pragma unroll
    for (int k = 0; k < kLagLW; ++k) B[(kLagLW * wave + k) * kChainCols + lane] = sum[k];
  __syncthreads();
}

// Wavefront 0 tells the others which columns go on, and whether any does.
__device__ __forceinline__ void lag_publish(int* s_live, int* s_any, int lane, bool live) {
  s_live[lane] = live;
  const bool any = __ballot(live) != 0;
  if (lane == 0) *s_any = any;
}

}  // namespace

}  // namespace tci
