// tci_chainquant.hip -- exact posterior quantiles of every chain column (mcmcstat's plims), selected on the
// device; the definition is in include/tci.h.
//
// One workgroup (4 wavefronts) takes a column tile of one chain (tci_chain_dev.h). The wavefronts split the rows
// (wavefront w the blocks of kChainRU rows w, w + 4, ..): they only count, and integer counts do not depend on the
// order of the rows, so the result is the same however the rows are split.
//
// An order statistic is found by an MSB-first radix selection on the 64-bit keys of tci_key.h, 8 bits a pass:
//   count  every key that matches the lane's prefix adds 1 to tab[next byte][lane] (an LDS table of 256 x 64
//          counters, 64 KiB; each column has its own counters, the four wavefronts add with ds_add_u32) and
//          enters the lane's running min / max of the matching keys;
//   walk   the lane sums its 256 counters up to the one that holds the rank: that byte joins the prefix, the
//          counts below it leave the rank. When min == max every matching key is the same key, which is then
//          the order statistic at once (a chain that rejects repeats its rows: most buckets end that way
//          after three or four passes instead of eight).
// The column needs the order statistics lo and lo + 1 of up to 16 probs. The host sorts the distinct ranks;
// the kernel takes them in ascending order and keeps, per column and per depth, the range of ranks of the bucket
// the last rank went through. The next rank starts below the deepest bucket that still holds it: ranks lo and
// lo + 1 share every pass but the last ones, and all of them when the two order statistics are one repeated
// value; ranks of different probs share the passes over sign, exponent and leading mantissa bits.
// The first pass of the first rank also tests every value for (x - x) == 0: a non-finite column is NaN.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "tci_chain_dev.h"
#include "tci_fp.h"
#include "tci_internal.h"
#include "tci_key.h"

namespace tci {

namespace {

constexpr int kCqBins = 256;   // 8 bits per pass
constexpr int kCqDepth = 8;    // passes that make a 64-bit key
constexpr int kCqRanks = 32;   // lo and lo + 1 of 16 probs

struct CqArgs {
  int32_t nq, n_ranks;
  int32_t rank[kCqRanks];  // ascending, distinct
  int32_t lo[16];
  double f[16];
};

// out: [n_chains][nq][ld + 1]
__global__ __launch_bounds__(kChainThreads) void k_cq_select(ChainView v, int64_t n, int tiles, CqArgs a,
                                                             double* __restrict__ out) {
  __shared__ uint32_t tab[kCqBins * kChainCols];                     // [bin][lane]
  __shared__ uint32_t stk_lo[kCqDepth * kChainCols], stk_hi[kCqDepth * kChainCols];  // [depth][lane]: the bucket's ranks
  __shared__ uint64_t red_mn[kChainWaves * kChainCols], red_mx[kChainWaves * kChainCols];
  __shared__ uint32_t red_bad[kChainWaves * kChainCols];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t c = blockIdx.x / tiles;
  const int64_t j = (int64_t)(blockIdx.x % tiles) * kChainCols + lane;
  const int64_t ldc = v.ld + 1;
  const bool in_out = j < ldc;
  bool live = chain_live(v, c, j);
  const ChainCol col = chain_col(v, c, j, live);
  double* outc = out + c * a.nq * ldc + j;
  const uint32_t nn = (uint32_t)n;

  uint64_t prev = 0, cur = 0;  // the keys of the last two ranks
  for (int i = 0; i < a.n_ranks; ++i) {
    const uint32_t t = (uint32_t)a.rank[i];
    // the deepest bucket of the last rank's path that holds rank t: depth bytes of its key are rank t's too
    int depth = 0;
    uint32_t base = 0, cnt = nn;
    if (i > 0) {
      __syncthreads();  // wavefront 0 wrote the last path
#pragma unroll
      for (int d = 0; d < kCqDepth; ++d) {
        const uint32_t lo = stk_lo[d * kChainCols + lane], hi = stk_hi[d * kChainCols + lane];
        if (depth == d && t >= lo && t < hi) {
          depth = d + 1;
          base = lo;
          cnt = hi - lo;
        }
      }
    }
    bool active = live && depth < kCqDepth;
    uint64_t prefix = depth == 0 ? 0 : cur & (~0ull << (64 - 8 * depth));
    prev = cur;
    // depth == kCqDepth: the same key again
    for (int d = 0; d < kCqDepth; ++d) {
      const bool mine = active && depth == d;
      if (__ballot(mine) == 0) continue;  // the same in all four wavefronts: their state is the same
      const int shift = 56 - 8 * d;
      __syncthreads();  // the last walk is over
      for (int b = wave; b < kCqBins; b += kChainWaves) tab[b * kChainCols + lane] = 0;
      __syncthreads();
      uint64_t mn = ~0ull, mx = 0;
      bool bad = false;
      for (int64_t r0 = (int64_t)wave * kChainRU; r0 < n; r0 += kChainWaves * kChainRU) {
        double x[kChainRU];
#pragma unroll
        for (int u = 0; u < kChainRU; ++u) x[u] = (mine && r0 + u < n) ? col.ptr[(r0 + u) * col.rs] : 0.0;
#pragma unroll
        for (int u = 0; u < kChainRU; ++u) {
          const uint64_t k = to_key(x[u]);
          bad |= !is_finite(x[u]);
          const bool m = mine && r0 + u < n && (d == 0 || ((k ^ prefix) >> (shift + 8)) == 0);
          if (m) {
            atomicAdd(&tab[(int)((k >> shift) & 255) * kChainCols + lane], 1u);
            mn = k < mn ? k : mn;
            mx = k > mx ? k : mx;
          }
        }
      }
      red_mn[wave * kChainCols + lane] = mn;
      red_mx[wave * kChainCols + lane] = mx;
      red_bad[wave * kChainCols + lane] = bad ? 1u : 0u;
      __syncthreads();
      // every wavefront walks for itself: the same counters, the same state
      uint32_t anybad = 0;
#pragma unroll
      for (int w = 0; w < kChainWaves; ++w) {
        const uint64_t m0 = red_mn[w * kChainCols + lane], m1 = red_mx[w * kChainCols + lane];
        mn = m0 < mn ? m0 : mn;
        mx = m1 > mx ? m1 : mx;
        anybad |= red_bad[w * kChainCols + lane];
      }
      if (mine && d == 0 && i == 0 && anybad) {  // a non-finite value: every quantile of the column is NaN
        live = false;
        active = false;
      } else if (mine && mn == mx) {  // one distinct key in the bucket: ranks base .. base + cnt - 1 are that key
        cur = mn;
        active = false;
        if (wave == 0)
          for (int e = d; e < kCqDepth; ++e) {
            stk_lo[e * kChainCols + lane] = base;
            stk_hi[e * kChainCols + lane] = base + cnt;
          }
      } else {
        uint32_t cum = base, blo = 0, bhi = 0;
        int byte = 0;
        bool found = false;
#pragma unroll 8
        for (int b = 0; b < kCqBins; ++b) {
          const uint32_t cb = tab[b * kChainCols + lane];
          const bool here = !found && t - cum < cb;  // cum <= t always
          if (here) {
            found = true;
            byte = b;
            blo = cum;
            bhi = cum + cb;
          }
          if (!found) cum += cb;
        }
        if (mine) {
          prefix |= (uint64_t)byte << shift;
          base = blo;
          cnt = bhi - blo;
          depth = d + 1;
          if (wave == 0) {
            stk_lo[d * kChainCols + lane] = blo;
            stk_hi[d * kChainCols + lane] = bhi;
          }
          if (d == kCqDepth - 1) {
            cur = prefix;
            active = false;
          }
        }
      }
    }
    // plims: y[lo] + f * (y[lo + 1] - y[lo]) once rank lo + 1 is known, y[n - 1] at the upper end
    if (wave == 0 && in_out) {
      for (int q = 0; q < a.nq; ++q) {
        const uint32_t lo = (uint32_t)a.lo[q];
        double r;
        if (lo + 1 < nn) {
          if (lo + 1 != t) continue;
          const double x0 = from_key(prev), x1 = from_key(cur);
          r = __dadd_rn(x0, __dmul_rn(a.f[q], __dsub_rn(x1, x0)));
        } else {
          if (lo != t) continue;
          r = from_key(cur);
        }
        outc[q * ldc] = live ? r : qnan();
      }
    }
  }
}

}  // namespace

int launch_chainquant(const double* chain, const double* s2, int64_t n_rows, int64_t n_chains, int64_t ld,
                      const int32_t* npar, const double* probs, int32_t nq, double* out, void* stream) {
  if (!chain || !probs || !out || n_rows < 1 || n_rows > ((int64_t)1 << 30) || n_chains < 1 || ld < 1 ||
      ld > ((int64_t)1 << 24) || nq < 1 || nq > 16)
    return TCI_EINVAL;
  const int64_t tiles = (ld + 1 + kChainCols - 1) / kChainCols;
  if (n_chains > ((int64_t)1 << 30) / tiles) return TCI_EINVAL;
  CqArgs a{};
  a.nq = nq;
  int32_t ranks[kCqRanks];
  int nr = 0;
  for (int q = 0; q < nq; ++q) {
    if (!(probs[q] >= 0.0 && probs[q] <= 1.0)) return TCI_EINVAL;
    const double h = (double)(n_rows - 1) * probs[q];
    const double lo = floor(h);
    a.lo[q] = (int32_t)lo;
    a.f[q] = h - lo;
    ranks[nr++] = a.lo[q];
    if ((int64_t)a.lo[q] + 1 < n_rows) ranks[nr++] = a.lo[q] + 1;
  }
  std::sort(ranks, ranks + nr);
  a.n_ranks = (int32_t)(std::unique(ranks, ranks + nr) - ranks);
  for (int k = 0; k < a.n_ranks; ++k) a.rank[k] = ranks[k];
  const ChainView v{chain, s2, npar, n_chains, ld};
  hipLaunchKernelGGL(k_cq_select, dim3((unsigned)(n_chains * tiles)), dim3(kChainThreads), 0, (hipStream_t)stream,
                     v, n_rows, (int)tiles, a, out);
  return hipGetLastError() == hipSuccess ? TCI_OK : TCI_EHIP;
}

}  // namespace tci
