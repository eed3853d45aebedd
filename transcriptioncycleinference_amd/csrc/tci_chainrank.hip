// tci_chainrank.hip -- the pooled sort of a group's column and what follows from it: pooled quantiles, the
// rank-normalised scores z (Vehtari et al. 2021), the scores of the folded column and the two tail indicator
// columns, written as chains of the chain's own layout so that launch_chainrhat / launch_chainess reduce them
// unchanged; the definition is in include/tci.h.
//
// One workgroup (8 wavefronts) takes one (group, column) of the chain (tci_chain_dev.h): the N = M n values of the
// group's chains, chains ascending, rows [0, n).
//   gather   element i = m n + r is row r of the group's m-th chain; its key is tci_key.h's 64-bit total order
//            (mode 1: of |x - med|). A non-finite value flags the column: everything it writes is NaN.
//   sort     keys only, by one bitonic network in its all-ascending form (the first stage of a merge of blocks
//            of k pairs i with its mirror image i ^ (k - 1), the later stages i with i + j): every comparator
//            leaves the smaller key at the lower index, so the network sorts any N when the indices >= N are
//            read as +infinity: those never move and are never stored. Two paths, chosen from N alone:
//            N <= kRankLdsCap  the keys sit in LDS, padded to the next power of two with ~0 (above every key);
//            N >  kRankLdsCap  the keys sit in a scratch slab of N keys in global memory. Tiles of kRankLdsCap keys
//                              are sorted in LDS; of every later merge the stages that span more than a tile run on
//                              the slab (comparators with a partner >= N are skipped) and the rest run tile by tile
//                              in LDS again.
//            The sorted keys are unique as a sequence, so the path cannot show in any result.
//   ranks    every thread looks its own elements up again: lt = lower bound, lt + eq = upper bound of the key in
//            the sorted keys (binary searches of at most 32 steps), R2 = 2 lt + eq + 1. No index array exists and
//            ties come out as average ranks.
//   z        p = (R2 - 0.75) / (2 N + 0.5), z = AS241's PPND16 of p, coefficient for coefficient the
//            expression of CPython's statistics.NormalDist.inv_cdf; the build has -ffp-contract=off, so every
//            Horner step is a multiplication, then an addition.
// Every loop is bounded by N, by a power of two >= N or by a bit count; none ends on a floating comparison.
#include <hip/hip_runtime.h>

#include <cmath>

#include "tci_chain_dev.h"
#include "tci_fp.h"
#include "tci_internal.h"
#include "tci_key.h"

namespace tci {

namespace {

constexpr int kCkThreads = 512;
constexpr int kCkLog2Cap = 13;
static_assert(kRankLdsCap == (1 << kCkLog2Cap), "the LDS tile is a power of two");

struct CkArgs {
  int32_t nq;
  double probs[16];
  double tail[2];
};

// Wichura's AS241 PPND16 as CPython's statistics._normal_dist_inv_cdf(p, 0.0, 1.0) writes it.
__device__ double ck_ppnd16(double p) {
  const double q = p - 0.5;
  double num, den;
  if (fabs(q) <= 0.425) {
    const double r = 0.180625 - q * q;
    num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
               4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
            1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
    den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
               2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
            4.2313330701600911252e+1) * r + 1.0);
    return 0.0 + (num / den) * 1.0;
  }
  double r = q <= 0.0 ? p : 1.0 - p;
  r = sqrt(-log(r));
  if (r <= 5.0) {
    r = r - 1.6;
    num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
               1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r +
            4.63033784615654529590e+0) * r + 1.42343711074968357734e+0);
    den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
               1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r +
            2.05319162663775882187e+0) * r + 1.0);
  } else {
    r = r - 5.0;
    num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
               2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r +
            5.46378491116411436990e+0) * r + 6.65790464350110377720e+0);
    den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
               7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
            5.99832206555888793690e-1) * r + 1.0);
  }
  double x = num / den;
  if (q < 0.0) x = -x;
  return 0.0 + x * 1.0;
}

__device__ __forceinline__ void ck_cmpx(uint64_t* a, uint64_t* b) {
  const uint64_t x = *a, y = *b;
  if (y < x) {
    *a = y;
    *b = x;
  }
}

// One stage of the network on the P = 2^lp keys of an LDS tile: comparator c of P / 2. flip: blocks of 2^lk keys,
// i against its mirror image; else i against i + 2^lj.
__device__ __forceinline__ void ck_lds_flip(uint64_t* t, int lp, int lk, int tid) {
  const int half = 1 << (lk - 1);
  for (int c = tid; c < (1 << (lp - 1)); c += kCkThreads) {
    const int b = (c >> (lk - 1)) << lk, o = c & (half - 1);
    ck_cmpx(&t[b + o], &t[b + (1 << lk) - 1 - o]);
  }
  __syncthreads();
}
__device__ __forceinline__ void ck_lds_step(uint64_t* t, int lp, int lj, int tid) {
  const int j = 1 << lj;
  for (int c = tid; c < (1 << (lp - 1)); c += kCkThreads) {
    const int i = ((c >> lj) << (lj + 1)) + (c & (j - 1));
    ck_cmpx(&t[i], &t[i + j]);
  }
  __syncthreads();
}
// The whole network on an LDS tile of 2^lp keys (written and synchronised by the caller).
__device__ void ck_lds_sort(uint64_t* t, int lp, int tid) {
  for (int lk = 1; lk <= lp; ++lk) {
    ck_lds_flip(t, lp, lk, tid);
    for (int lj = lk - 2; lj >= 0; --lj) ck_lds_step(t, lp, lj, tid);
  }
}

// The element i = m n + r of a (group, column): its value.
struct CkCol {
  const double* base;    // column j of chain 0, row 0 (or s2 of chain 0)
  int64_t cs, rs;        // strides of a chain and of a row
  const int32_t* list;   // the group's chains
  int64_t n;
  __device__ __forceinline__ int64_t at(int64_t i) const { return (int64_t)list[i / n] * cs + (i % n) * rs; }
};

// mode 0: ranks of x, and the pooled quantiles into qbuf; mode 1: ranks of |x - med|; mode 2, 3: the indicator
// x <= q_lo, x <= q_hi. qbuf: [n_groups][nq + 3][ld + 1] = probs' quantiles, then med, q_lo, q_hi. zc, zs2: the
// transformed chain, laid out as the chain. gkeys: n_blocks slabs of gstride keys (the global path; null without).
__global__ __launch_bounds__(kCkThreads) void k_ck_rank(ChainView v, int64_t n, int mode, int lp_lds,
                                                         const int32_t* __restrict__ g_off,
                                                         const int32_t* __restrict__ g_list, CkArgs a,
                                                         double* __restrict__ qbuf, uint64_t* __restrict__ gkeys,
                                                         int64_t gstride, double* __restrict__ zc,
                                                         double* __restrict__ zs2) {
  extern __shared__ __align__(16) uint64_t ck_lds[];
  const int tid = threadIdx.x;
  const int64_t ldc = v.ld + 1;
  const int64_t g = (int64_t)blockIdx.x / ldc, j = (int64_t)blockIdx.x % ldc;
  const int32_t b0 = g_off[g];
  const int64_t M = g_off[g + 1] - b0;
  if (M < 1) return;
  const int32_t* list = g_list + b0;
  if (!chain_live(v, list[0], j)) return;  // padding: stays NaN
  const int64_t N = M * n;
  const bool s2col = j == v.ld;
  const ChainCol col0 = chain_col(v, 0, j, true);
  const CkCol col{col0.ptr, s2col ? 1 : v.ld, col0.rs, list, n};
  double* const zout = s2col ? zs2 : zc + j;  // the same strides
  const int nqq = a.nq + 3;
  double* const qg = qbuf + (g * nqq) * ldc + j;

  if (mode >= 2) {  // the indicator of the pooled tail quantile: no sort
    const double q = qg[(a.nq + mode - 1) * ldc];
    for (int64_t i = tid; i < N; i += kCkThreads) {
      const int64_t o = col.at(i);
      zout[o] = q != q ? qnan() : (col.base[o] <= q ? 1.0 : 0.0);
    }
    return;
  }

  const double med = mode == 1 ? qg[a.nq * ldc] : 0.0;
  auto value = [&](int64_t i) {
    const double x = col.base[col.at(i)];
    return mode == 1 ? fabs(x - med) : x;
  };
  bool bad = false;
  const uint64_t* sorted;
  if (N <= kRankLdsCap) {
    const int P = 1 << lp_lds;  // >= N: the launch sized the tile for the largest group below the cap
    int lp = 1;
    while ((1 << lp) < N) ++lp;  // at most kCkLog2Cap steps
    for (int i = tid; i < P; i += kCkThreads) {
      uint64_t k = ~0ull;
      if (i < N) {
        const double x = value(i);
        bad |= !is_finite(x);
        k = to_key(x);
      }
      ck_lds[i] = k;
    }
    __syncthreads();
    ck_lds_sort(ck_lds, lp, tid);
    sorted = ck_lds;
  } else {
    constexpr int64_t T = kRankLdsCap;
    uint64_t* gk = gkeys + (int64_t)blockIdx.x * gstride;
    for (int64_t t0 = 0; t0 < N; t0 += T) {  // every tile sorted in LDS
      for (int i = tid; i < T; i += kCkThreads) {
        uint64_t k = ~0ull;
        if (t0 + i < N) {
          const double x = value(t0 + i);
          bad |= !is_finite(x);
          k = to_key(x);
        }
        ck_lds[i] = k;
      }
      __syncthreads();
      ck_lds_sort(ck_lds, kCkLog2Cap, tid);
      for (int i = tid; i < T; i += kCkThreads)
        if (t0 + i < N) gk[t0 + i] = ck_lds[i];
      __syncthreads();
    }
    int lpt = kCkLog2Cap + 1;
    while (((int64_t)1 << lpt) < N) ++lpt;  // N < 2^31
    for (int lk = kCkLog2Cap + 1; lk <= lpt; ++lk) {
      const int64_t ncmp = (int64_t)1 << (lpt - 1), half = (int64_t)1 << (lk - 1);
      for (int64_t c = tid; c < ncmp; c += kCkThreads) {  // the flip of blocks of 2^lk keys
        const int64_t b = (c >> (lk - 1)) << lk, o = c & (half - 1);
        const int64_t i = b + o, p = b + ((int64_t)1 << lk) - 1 - o;
        if (p < N) ck_cmpx(&gk[i], &gk[p]);
      }
      __syncthreads();
      for (int lj = lk - 2; lj >= kCkLog2Cap; --lj) {  // the stages that span more than a tile
        const int64_t jj = (int64_t)1 << lj;
        for (int64_t c = tid; c < ncmp; c += kCkThreads) {
          const int64_t i = ((c >> lj) << (lj + 1)) + (c & (jj - 1));
          if (i + jj < N) ck_cmpx(&gk[i], &gk[i + jj]);
        }
        __syncthreads();
      }
      for (int64_t t0 = 0; t0 < N; t0 += T) {  // the rest, tile by tile
        for (int i = tid; i < T; i += kCkThreads) ck_lds[i] = t0 + i < N ? gk[t0 + i] : ~0ull;
        __syncthreads();
        for (int lj = kCkLog2Cap - 1; lj >= 0; --lj) ck_lds_step(ck_lds, kCkLog2Cap, lj, tid);
        for (int i = tid; i < T; i += kCkThreads)
          if (t0 + i < N) gk[t0 + i] = ck_lds[i];
        __syncthreads();
      }
    }
    sorted = gk;
  }
  bad = __syncthreads_or(bad) != 0;

  if (mode == 0 && tid < nqq) {  // plims on the pooled order, n := N
    const double p = tid < a.nq ? a.probs[tid] : tid == a.nq ? 0.5 : a.tail[tid - a.nq - 1];
    const double h = (double)(N - 1) * p;
    const double fl = floor(h);
    const double f = h - fl;
    const int64_t lo = (int64_t)fl;
    double r;
    if (lo + 1 < N) {
      const double x0 = from_key(sorted[lo]), x1 = from_key(sorted[lo + 1]);
      r = x0 + f * (x1 - x0);
    } else {
      r = from_key(sorted[N - 1]);
    }
    qg[tid * ldc] = bad ? qnan() : r;
  }

  const double den = (double)(2 * N) + 0.5;
  for (int64_t i = tid; i < N; i += kCkThreads) {
    const int64_t o = col.at(i);
    double z = qnan();
    if (!bad) {
      const double x = col.base[o];
      const uint64_t k = to_key(mode == 1 ? fabs(x - med) : x);
      int64_t lo = 0, hi = N;
      for (int it = 0; it < 32 && lo < hi; ++it) {  // keys below k
        const int64_t mid = (lo + hi) >> 1;
        if (sorted[mid] < k) lo = mid + 1;
        else hi = mid;
      }
      const int64_t lt = lo;
      hi = N;
      for (int it = 0; it < 32 && lo < hi; ++it) {  // keys not above k
        const int64_t mid = (lo + hi) >> 1;
        if (sorted[mid] <= k) lo = mid + 1;
        else hi = mid;
      }
      const int64_t R2 = lt + lo + 1;  // 2 lt + eq + 1
      z = ck_ppnd16(((double)R2 - 0.75) / den);
    }
    zout[o] = z;
  }
}

// The quiet NaN the other reductions write, in every entry.
__global__ __launch_bounds__(256) void k_ck_fill(double* __restrict__ p, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = qnan();
}

}  // namespace

int launch_chainrank_fill(double* p, size_t n, void* stream) {
  if (!p) return TCI_EINVAL;
  if (n == 0) return TCI_OK;
  const size_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(k_ck_fill, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream, p, n);
  return hipGetLastError() == hipSuccess ? TCI_OK : TCI_EHIP;
}

int chainrank_scratch_keys(int64_t n_rows, int64_t ld, int64_t n_groups, const int32_t* g_off, int64_t* stride,
                           size_t* keys) {
  if (n_rows < 1 || ld < 1 || n_groups < 1 || !g_off || !stride || !keys) return TCI_EINVAL;
  int64_t maxN = 0;
  for (int64_t g = 0; g < n_groups; ++g) {
    const int64_t M = g_off[g + 1] - g_off[g];
    if (M > (((int64_t)1 << 31) - 1) / n_rows) return TCI_ERANGE;  // N = M n below 2^31
    maxN = M * n_rows > maxN ? M * n_rows : maxN;
  }
  if ((long double)n_groups * (ld + 1) > 2147483647.0L) return TCI_ERANGE;
  *stride = maxN > kRankLdsCap ? maxN : 0;
  if ((long double)*stride * n_groups * (ld + 1) > (long double)((size_t)1 << 43)) return TCI_ENOMEM;  // 2^46 bytes
  *keys = (size_t)*stride * (size_t)n_groups * (size_t)(ld + 1);
  return TCI_OK;
}

int launch_chainrank(const double* chain, const double* s2, int64_t n_rows, int64_t n_chains, int64_t ld,
                     const int32_t* npar, int64_t n_groups, const int32_t* g_off_host, const int32_t* g_off,
                     const int32_t* g_list, int mode, const double* probs, int32_t nq, double tail_lo, double tail_hi,
                     double* qbuf, void* gkeys, double* zc, double* zs2, void* stream) {
  if (!chain || !g_off_host || !g_off || !g_list || !probs || !qbuf || !zc || (s2 && !zs2) || mode < 0 || mode > 3 ||
      n_chains < 1 || nq < 1 || nq > 16 || ld > ((int64_t)1 << 24))
    return TCI_EINVAL;
  int64_t stride = 0;
  size_t keys = 0;
  const int rc = chainrank_scratch_keys(n_rows, ld, n_groups, g_off_host, &stride, &keys);
  if (rc != TCI_OK) return rc;
  if (keys && !gkeys) return TCI_EINVAL;
  int lp = 1;  // the LDS tile: the largest group below the cap, or the cap itself
  for (int64_t g = 0; g < n_groups; ++g) {
    const int64_t N = (int64_t)(g_off_host[g + 1] - g_off_host[g]) * n_rows;
    while (lp < kCkLog2Cap && ((int64_t)1 << lp) < N) ++lp;
  }
  const size_t lds = mode >= 2 ? 0 : sizeof(uint64_t) << lp;
  if (ensure_dyn_lds((const void*)k_ck_rank, lds) != TCI_OK) return TCI_EHIP;
  CkArgs a{};
  a.nq = nq;
  for (int q = 0; q < nq; ++q) a.probs[q] = probs[q];
  a.tail[0] = tail_lo;
  a.tail[1] = tail_hi;
  const ChainView v{chain, s2, npar, n_chains, ld};
  hipLaunchKernelGGL(k_ck_rank, dim3((unsigned)(n_groups * (ld + 1))), dim3(kCkThreads), lds, (hipStream_t)stream, v,
                     n_rows, mode, lp, g_off, g_list, a, qbuf, (uint64_t*)gkeys, stride, zc, zs2);
  return hipGetLastError() == hipSuccess ? TCI_OK : TCI_EHIP;
}

}  // namespace tci
