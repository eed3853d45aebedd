// tci_loocheck.hip -- PSIS-LOO of every datum under the S posterior samples of a chain: the tail of the importance
// ratios selected exactly, a generalised-Pareto fit to it, the smoothed tail, and the leave-one-out log predictive
// density with its Pareto k; the definition is in include/tci.h.
//
// The forward kernel leaves the S simulated rows of a chain in HBM (tci_loocheck, tci_api.cpp). One workgroup of one
// wavefront per (selected chain, dye, tile of 64 time points); lane l is time point 64 * tile + l, so a row read is one
// 512 B segment, as in k_fitcheck. A lane owns its point from the first row to the outputs: nothing crosses lanes, so
// there is no barrier, and a point's bits follow from its own samples, data and S alone.
//
// Selecting the M largest of S ratios per point (M <= 192, S <= 4096). The ratios of a 64-point tile are S x 512 B
// (2 MiB at the cap): they do not fit a CU's LDS, and lanes along the sample axis would break the coalesced reads. So
// the rows are streamed and every lane keeps a min-heap of the M largest (key, s) pairs seen so far in LDS, laid out
// [M][64]: lane l touches only banks 2 l and 2 l + 1 (mod 64) whatever its heap index, so diverging indices cost no
// bank conflict. The key is tci_key.h's order-preserving map of the double, compared before s: the total order of the
// contract. A sample below the root leaves at once; the largest key that left (or was evicted) is `cut`. A heap sort in
// place then gives tail_1 .. tail_M. LDS: M x 64 x (8 + 2) B for the heap (120 KiB at M = 192, 42.5 KiB at S = 500) and
// G x 64 x 8 B (<= 21.5 KiB) for the profile log-likelihoods L_g: at most 141.5 KiB of the CU's 160 KiB.
//
// Five passes over the rows (the second to the fifth find them in L2 / MALL): (1) max and min of ll and the finiteness
// of the rows; (2) SUM exp(ll - m) for lppd, with k_fitcheck's operations and order (the same bits), and the heap;
// then the fit, for which x_j = exp(tail_j) - ec is restated from the key inside every sum (LDS has no room for a second
// [M][64] array at the cap); the smoothed values overwrite the keys and a second heap sort orders the tail by s, so
// that (3) and (4), which walk the samples in ascending s, meet the tail entries in turn with no search: (3) the maximum
// of lw + ll, (4) the two sums of the log-sum-exps.
#include <hip/hip_runtime.h>

#include <cmath>

#include "tci_fp.h"
#include "tci_internal.h"
#include "tci_key.h"

namespace tci {

namespace {

constexpr int kLcLanes = 64;  // time points per tile: one per lane, one wavefront per workgroup
constexpr int kLcSeg = 64;    // samples per segment (include/tci.h: the order of every SUM_s)
constexpr int kLcU = 8;       // rows a wavefront loads together

struct LcEnt {
  uint64_t k;  // a key, or the bits of a double
  uint32_t s;
};

// The heap of one lane: entry i at [i][lane].
struct LcHeap {
  uint64_t* val;
  uint16_t* idx;
  int lane;
  __device__ __forceinline__ LcEnt get(int i) const {
    return LcEnt{val[i * kLcLanes + lane], (uint32_t)idx[i * kLcLanes + lane]};
  }
  __device__ __forceinline__ void put(int i, LcEnt e) const {
    val[i * kLcLanes + lane] = e.k;
    idx[i * kLcLanes + lane] = (uint16_t)e.s;
  }
};

// Does a belong nearer the root than b? BY_S = false: the smaller (key, s) (a min-heap of the contract's order);
// BY_S = true: the larger s (a max-heap; s is unique).
template <bool BY_S>
__device__ __forceinline__ bool lc_before(LcEnt a, LcEnt b) {
  if (BY_S) return a.s > b.s;
  return a.k < b.k || (a.k == b.k && a.s < b.s);
}

// Put e into the hole at i of the heap's first n entries (every index read or written is below n).
template <bool BY_S>
__device__ __forceinline__ void lc_sift(const LcHeap& h, int i, int n, LcEnt e) {
  for (;;) {
    int c = 2 * i + 1;
    if (c >= n) break;
    LcEnt ce = h.get(c);
    if (c + 1 < n) {
      const LcEnt c1 = h.get(c + 1);
      if (lc_before<BY_S>(c1, ce)) {
        ce = c1;
        c = c + 1;
      }
    }
    if (!lc_before<BY_S>(ce, e)) break;
    h.put(i, ce);
    i = c;
  }
  h.put(i, e);
}

template <bool BY_S>
__device__ __forceinline__ void lc_build(const LcHeap& h, int n) {
  for (int i = n / 2 - 1; i >= 0; --i) lc_sift<BY_S>(h, i, n, h.get(i));
}

// Heap sort in place: the root goes to the end of the shrinking heap, so afterwards entry n - 1 is the one that
// lc_before puts first and entry 0 the one it puts last: BY_S = false: descending (key, s); BY_S = true: ascending s.
template <bool BY_S>
__device__ __forceinline__ void lc_sort(const LcHeap& h, int n) {
  for (int m = n - 1; m >= 1; --m) {
    const LcEnt last = h.get(m);
    h.put(m, h.get(0));
    lc_sift<BY_S>(h, 0, m, last);
  }
}

// ll_s as k_fitcheck has it: every operation rounded once (the build has -ffp-contract=off)
__device__ __forceinline__ double lc_ll(double y, double f, double sd, double lg) {
  const double r = y - f;
  const double z = r / sd;
  const double zz = z * z;
  return -0.5 * (lg + zz);
}

// f(s, sim value, ll) for s = 0 .. S - 1 in ascending order, kLcU rows loaded together.
template <class F>
__device__ __forceinline__ void lc_rows(int S, const double* col, int64_t ld, bool live, const double* sdk,
                                        const double* lgk, double y, F&& f) {
  for (int s0 = 0; s0 < S; s0 += kLcU) {
    double v[kLcU];
#pragma unroll
    for (int u = 0; u < kLcU; ++u) v[u] = (live && s0 + u < S) ? col[(int64_t)(s0 + u) * ld] : 0.0;
#pragma unroll
    for (int u = 0; u < kLcU; ++u)
      if (s0 + u < S) f(s0 + u, v[u], lc_ll(y, v[u], sdk[s0 + u], lgk[s0 + u]));
  }
}

struct LcTable {
  double c[kLcMaxG];  // c[g - 1] = 1 - sqrt(G / (g - 0.5)), the host's
};

// sim: [n_sel * S][ld_out] rows of one dye per pointer; sd, lg: [n_sel * S]; out: [n_sel][2][4][ld_out].
__global__ __launch_bounds__(kLcLanes) void k_loocheck(const CellMeta* __restrict__ cells,
                                                       const PointRec* __restrict__ points, int64_t cell_stride,
                                                       const int32_t* __restrict__ row_cell,
                                                       const double* __restrict__ sim0,
                                                       const double* __restrict__ sim1, const double* __restrict__ sd,
                                                       const double* __restrict__ lg, int S, int M, int G,
                                                       int64_t ld_out, int tiles, double logS, LcTable tab,
                                                       double* __restrict__ out) {
  extern __shared__ uint64_t lc_lds[];
  const int lane = threadIdx.x;
  const int64_t bid = blockIdx.x;
  const int tile = (int)(bid % tiles);
  const int64_t rest = bid / tiles;
  const int dye = (int)(rest & 1);
  const int64_t k = rest >> 1;
  const int32_t cell = row_cell[k * S];
  const int N = cells[cell].n;
  const int64_t j = (int64_t)tile * kLcLanes + lane;
  double* o = out + (k * 2 + dye) * 4 * ld_out + j;
  if ((int64_t)tile * kLcLanes >= N) {  // a tile of padding only
    if (j < ld_out)
      for (int q = 0; q < 4; ++q) o[q * ld_out] = qnan();
    return;
  }
  // LDS: val [M][64] (8 B), Lg [G][64] (8 B), idx [M][64] (2 B)
  uint64_t* val = lc_lds;
  double* Lg = (double*)(lc_lds + (size_t)M * kLcLanes);
  uint16_t* idx = (uint16_t*)(Lg + (size_t)G * kLcLanes);
  const LcHeap h{val, idx, lane};

  const bool live = j < N;  // the forward launch wrote sim[.., j] for j < N only
  const double* col = (dye ? sim1 : sim0) + k * S * ld_out + j;
  const double* sdk = sd + k * S;
  const double* lgk = lg + k * S;
  double y = 0.0;
  if (live) {
    const PointRec& p = points[(int64_t)cell * cell_stride + j];
    y = dye ? p.y2 : p.y1;
  }
  const double dM = (double)M;

  // ---- pass 1: max and min of ll, and whether every row is finite here
  double m = -INFINITY, mx = -INFINITY;  // mx = max_s (-ll_s)
  bool bad = false;
  lc_rows(S, col, ld_out, live, sdk, lgk, y, [&](int, double f, double ll) {
    bad |= !is_finite(f);
    m = ll > m ? ll : m;
    const double nl = -ll;
    mx = nl > mx ? nl : mx;
  });

  // a tile with no scored point (the same for the whole wavefront): NaN everywhere, no selection and no fit
  if (__ballot(live && is_finite(y) && !bad) == 0) {
    if (j < ld_out)
      for (int q = 0; q < 4; ++q) o[q * ld_out] = qnan();
    return;
  }

  // ---- pass 2: SUM exp(ll - m) (k_fitcheck's lppd), and the M largest lr_s = (-ll_s) - mx by (key, s)
  double tot = 0.0, acc = 0.0;
  uint64_t cutk = 0;  // below every key
  lc_rows(S, col, ld_out, live, sdk, lgk, y, [&](int s, double, double ll) {
    acc = acc + exp(ll - m);
    if ((s & (kLcSeg - 1)) == kLcSeg - 1 || s == S - 1) {
      tot = tot + acc;
      acc = 0.0;
    }
    const LcEnt e{to_key((-ll) - mx), (uint32_t)s};
    if (s < M) {
      h.put(s, e);
      if (s == M - 1) lc_build<false>(h, M);
    } else {
      const LcEnt root = h.get(0);
      uint64_t gone = e.k;
      if (lc_before<false>(root, e)) {
        gone = root.k;
        lc_sift<false>(h, 0, M, e);
      }
      cutk = gone > cutk ? gone : cutk;
    }
  });
  const double lppd = (m + log(tot)) - logS;
  lc_sort<false>(h, M);  // tail_j = entry M - j, j = 1 .. M
  const double cut = from_key(cutk);

  // ---- the generalised-Pareto fit
  const double ec = exp(cut);
  auto x_at = [&](int jj) { return exp(from_key(val[(M - jj) * kLcLanes + lane])) - ec; };  // x_jj, jj = 1 .. M
  const double xM = x_at(M), x1 = x_at(1);
  // spelled out: is_finite(xM) here makes the compiler order the whole kernel differently
  bool degenerate = !(xM > 0.0) || (xM - xM) != 0.0 || x1 < 0.0;
  double khat = INFINITY, sigma = 0.0;
  {
    const double xq = x_at((M + 2) / 4);  // floor(M / 4 + 0.5)
    const double ixM = 1.0 / xM, xq3 = 3.0 * xq;
    for (int g = 0; g < G; ++g) {
      const double bg = ixM + tab.c[g] / xq3;
      double sum = 0.0;
      for (int jj = 1; jj <= M; ++jj) sum = sum + log1p(-bg * x_at(jj));
      const double kg = sum / dM;
      Lg[g * kLcLanes + lane] = dM * ((log(-bg / kg) + (-kg)) - 1.0);
    }
    double b = 0.0;
    for (int g = 0; g < G; ++g) {
      const double Lgg = Lg[g * kLcLanes + lane];
      double den = 0.0;
      for (int hh = 0; hh < G; ++hh) den = den + exp(Lg[hh * kLcLanes + lane] - Lgg);
      const double wg = 1.0 / den;
      b = b + (ixM + tab.c[g] / xq3) * wg;
    }
    double sum = 0.0;
    for (int jj = 1; jj <= M; ++jj) sum = sum + log1p(-b * x_at(jj));
    const double kk = sum / dM;
    sigma = -kk / b;
    const double kh = (kk * dM + 5.0) / (double)(M + 10);
    if (!is_finite(kh) || !is_finite(sigma)) degenerate = true;
    if (!degenerate) khat = kh;
  }

  // ---- the smoothed tail over the keys (the bits of lw), the largest lw, and the tail ordered by s
  double mB = cut;
  for (int jj = 1; jj <= M; ++jj) {
    const int at = (M - jj) * kLcLanes + lane;
    double t = from_key(val[at]);
    if (!degenerate) {
      const double p = ((double)jj - 0.5) / dM;
      const double q = sigma * expm1(-khat * log1p(-p)) / khat;
      const double sm = log(q + ec);
      t = (sm < 0.0 || sm != sm) ? sm : 0.0;  // min(sm, 0.0), a NaN kept
    }
    mB = t > mB ? t : mB;
    val[at] = (uint64_t)__double_as_longlong(t);
  }
  lc_build<true>(h, M);
  lc_sort<true>(h, M);

  // ---- pass 3: max_s (lw_s + ll_s)
  double mA = -INFINITY;
  int p = 0;
  uint32_t next = idx[lane];
  auto lw_of = [&](int s, double ll) {
    double lw = (-ll) - mx;
    if ((uint32_t)s == next) {
      lw = __longlong_as_double((long long)val[p * kLcLanes + lane]);
      ++p;
      next = p < M ? (uint32_t)idx[p * kLcLanes + lane] : 0xFFFFFFFFu;
    }
    return lw;
  };
  lc_rows(S, col, ld_out, live, sdk, lgk, y, [&](int s, double, double ll) {
    const double a = lw_of(s, ll) + ll;
    mA = a > mA ? a : mA;
  });

  // ---- pass 4: SUM exp((lw + ll) - mA) and SUM exp(lw - mB)
  double totA = 0.0, totB = 0.0, accA = 0.0, accB = 0.0;
  p = 0;
  next = idx[lane];
  lc_rows(S, col, ld_out, live, sdk, lgk, y, [&](int s, double, double ll) {
    const double lw = lw_of(s, ll);
    accA = accA + exp((lw + ll) - mA);
    accB = accB + exp(lw - mB);
    if ((s & (kLcSeg - 1)) == kLcSeg - 1 || s == S - 1) {
      totA = totA + accA;
      totB = totB + accB;
      accA = 0.0;
      accB = 0.0;
    }
  });

  if (j < ld_out) {
    const bool scored = live && is_finite(y) && !bad;
    const double elpd = (mA + log(totA)) - (mB + log(totB));
    o[0] = scored ? elpd : qnan();
    o[ld_out] = scored ? lppd : qnan();
    o[2 * ld_out] = scored ? lppd - elpd : qnan();
    o[3 * ld_out] = scored ? khat : qnan();
  }
}

int64_t lc_tiles(int64_t ld_out) { return (ld_out + kLcLanes - 1) / kLcLanes; }

}  // namespace

int loocheck_tail(int64_t S, int32_t* M, int32_t* G) {
  if (S < 32 || S > 4096) return TCI_EINVAL;
  const int64_t a = S / 5, b = (int64_t)std::ceil(3.0 * std::sqrt((double)S));
  *M = (int32_t)(a < b ? a : b);
  *G = 30 + (int32_t)std::floor(std::sqrt((double)*M));
  return TCI_OK;
}

int loocheck_max_cells(int64_t S, int64_t ld_out, int64_t* max_cells) {
  // one launch: 2 * chains * tiles workgroups in grid.x, and chains * S rows in the forward launch's grid.x
  const int64_t by_grid = ((int64_t)1 << 30) / (2 * lc_tiles(ld_out)), by_rows = ((int64_t)1 << 30) / S;
  *max_cells = by_grid < by_rows ? by_grid : by_rows;
  return *max_cells >= 1 ? TCI_OK : TCI_EINVAL;
}

int launch_loocheck(const KParams& kp, const int32_t* row_cell, const double* sim0, const double* sim1,
                    const double* sd, const double* lg, int64_t n_sel, int64_t S, int64_t ld_out, double logS,
                    double* out, void* stream) {
  if (n_sel <= 0) return TCI_OK;
  int32_t M = 0, G = 0;
  if (loocheck_tail(S, &M, &G) != TCI_OK || ld_out < 1) return TCI_EINVAL;
  if (M < 6 || M > kLcMaxM || M > S / 5 || G < 1 || G > kLcMaxG) return TCI_EINVAL;  // what the kernel's indices rely on
  const int64_t tiles = lc_tiles(ld_out);
  if (tiles > ((int64_t)1 << 30) || 2 * n_sel > ((int64_t)1 << 30) / tiles) return TCI_EINVAL;
  const size_t lds = (size_t)kLcLanes * ((size_t)M * 10 + (size_t)G * 8);
  if (lds > (size_t)160 * 1024) return TCI_EINVAL;
  if (ensure_dyn_lds((const void*)k_loocheck, lds) != TCI_OK) return TCI_EHIP;
  LcTable tab{};
  for (int g = 1; g <= G; ++g) tab.c[g - 1] = 1.0 - std::sqrt((double)G / ((double)g - 0.5));
  hipLaunchKernelGGL(k_loocheck, dim3((unsigned)(2 * n_sel * tiles)), dim3(kLcLanes), lds, (hipStream_t)stream,
                     kp.cells, kp.points, kp.cell_stride, row_cell, sim0, sim1, sd, lg, (int)S, (int)M, (int)G, ld_out,
                     (int)tiles, logS, tab, out);
  return hipGetLastError() == hipSuccess ? TCI_OK : TCI_EHIP;
}

}  // namespace tci
