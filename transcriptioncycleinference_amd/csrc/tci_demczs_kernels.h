// tci_demczs_kernels.h -- the two kernels of the DE-MC(zs) sampler, k_zs_propose and k_zs_decide, as templates; the
// description is tci_demczs.hip's. Two translation units include this file and instantiate what they launch:
// tci_demczs.hip the kernels without kBounds (tci_demczs_run), tci_demczs_bounds.hip the ones with it
// (tci_demczs_run_bounds). Each unit is a code object of its own, so the code object that holds the kernels of the
// existing entry points holds nothing else.
#ifndef TCI_DEMCZS_KERNELS_H_
#define TCI_DEMCZS_KERNELS_H_

#include <hip/hip_runtime.h>
#include <math.h>

#include "tci_fp.h"
#include "tci_gamma.h"
#include "tci_internal.h"
#include "tci_prior.h"
#include "tci_rng.h"

namespace tci {

namespace {

constexpr int kZsThreads = 256;
constexpr int kZsWaves = kZsThreads / 64;
constexpr int kZsDecThreads = 1024;  // k_zs_decide: one workgroup per cell
constexpr int kZsDecWaves = kZsDecThreads / 64;
constexpr int kZsMaxPop = 4096;
// 9-12 are the DE-MC sampler's (tci_demc.hip)
constexpr uint32_t kPurposeIndex = 13, kPurposeCoord = 14, kPurposeAccept = 15, kPurposeSigma = 16;
// the coordinate counter i * 4096 + j, as k_demc_propose's
static_assert(7 + TCI_MAX_POINTS <= 4096, "the coordinate counter of k_zs_propose");
static_assert((7 + TCI_MAX_POINTS + 63) / 64 <= 64, "the crossing mask of k_zs_propose");

// m(w, n) of include/tci.h: a word scaled to [0, n)
__device__ __forceinline__ uint32_t zs_scale(uint32_t w, uint32_t n) { return (uint32_t)(((uint64_t)w * n) >> 32); }

// The 64 lane partials by the xor butterfly: addition commutes bitwise, so every lane holds the same value.
__device__ __forceinline__ double zs_sum64(double p) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) p = p + __shfl_xor(p, d, 64);
  return p;
}

// The trailing argument of a kBounds instantiation; the instantiations without the flag take none, so their signature
// and kernel-argument segment are what they were before the flag existed.
struct ZsNone {};
__device__ __forceinline__ ZsNone zs_extra() { return {}; }
template <typename T>
__device__ __forceinline__ const T& zs_extra(const T& x) { return x; }

// kInit: the prior of every chain's start (nothing but pop, mu and sig is read). Else: the trial of every chain in
// generation gen, from the first M_g rows of its cell's archive. B = n_sel * n_pop rows either way.
// kBounds (tci_demczs_run_bounds; bx, the one trailing argument, exists with it alone): the
// census and the oriented reflection ride in pass 2 of either move, so the row is walked no more often. Row b's
// counters and orientation bytes are loaded and stored by row b's wavefront alone, lane l owning j = l, l + 64, ..
template <bool kInit, bool kBounds, typename... Extra>
__global__ __launch_bounds__(kZsThreads) void k_zs_propose(
    const CellMeta* __restrict__ cells, const int32_t* __restrict__ cell_id, const int64_t* __restrict__ keys,
    const double* __restrict__ pop, const double* __restrict__ arch, const double* __restrict__ lower,
    const double* __restrict__ upper, const double* __restrict__ mu, const double* __restrict__ sig,
    const double* __restrict__ jitter, uint32_t n_pop, uint32_t M_g, int64_t M_cap, int64_t ld, int64_t B, int64_t gen,
    int jump, uint64_t seed, double gamma0, double CR, double p_snooker, double* trial, double* __restrict__ pri,
    double* __restrict__ ljac, uint8_t* __restrict__ move, uint8_t* __restrict__ active, Extra... extra) {
  static_assert(sizeof...(Extra) == (kBounds ? 1 : 0), "one ZsBounds with kBounds, nothing without");
  const auto& bx = zs_extra(extra...);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.x * kZsWaves + wave;
  if (b >= B) return;                              // the whole wavefront
  const uint32_t k = (uint32_t)b / n_pop, i = (uint32_t)b % n_pop;  // B < 2^31 (the host checked): 32-bit divisions
  const int P = 7 + cells[cell_id[k]].n;           // <= ld (the host checked)
  if (kInit) {
    const double tot = prior_sum64(pop + b * ld, mu + (int64_t)k * ld, sig + (int64_t)k * ld, P, lane);
    if (lane == 0) pri[b] = tot;
    return;
  }
  const int64_t key = keys[k];
  const uint4 w = rng(seed, key, gen, kPurposeIndex, i);
  const uint4 q = rng(seed, key, gen, kPurposeIndex, (uint32_t)kZsMaxPop + i);
  const uint32_t a = zs_scale(w.x, M_g);           // M_g >= 3 (the host checked m0)
  uint32_t c = zs_scale(w.y, M_g - 1);
  c += c >= a;
  const bool snk = u01(q.x, q.y) < p_snooker;      // every lane alike: wave-uniform
  const double* Z = arch + (int64_t)k * M_cap * ld;
  const double* xi = pop + b * ld;
  const double* lo = lower + (int64_t)k * ld;
  const double* up = upper + (int64_t)k * ld;
  double* tr = trial + b * ld;
  bool oob = false;
  double lj = 0.0;
  int n_left = 0, n_refl = 0;  // kBounds: this lane's coordinates of the raw trial outside, and reflected
  if (snk) {
    const uint32_t mn = a < c ? a : c, mx = a < c ? c : a;
    uint32_t e = zs_scale(w.w, M_g - 2);
    e += e >= mn;
    e += e >= mx;
    const double gs = 1.2 + u01(q.z, q.w);
    const double* z = Z + (int64_t)e * ld;
    const double* z1 = Z + (int64_t)a * ld;
    const double* z2 = Z + (int64_t)c * ld;
    double pD = 0.0, pA = 0.0;
    for (int j = lane; j < P; j += 64) {
      const double d = xi[j] - z[j];
      const double dd = d * d;
      pD = pD + dd;
      const double g = z1[j] - z2[j];
      const double gd = g * d;
      pA = pA + gd;
    }
    const double D = zs_sum64(pD), A = zs_sum64(pA);
    if (D == 0.0 || !is_finite(D)) {  // a null move: the chain drew its own copy, or D is Inf or NaN
      // the trial row is left as an earlier generation wrote it, on purpose: active = 0 keeps every reader off it
      if (lane == 0) {
        pri[b] = qnan();
        ljac[b] = qnan();
        move[b] = 2;
        active[b] = 0;
      }
      return;  // the whole wavefront
    }
    const double r = A / D;
    const double s = gs * r;
    double pE = 0.0;
    for (int64_t j = lane; j < ld; j += 64) {
      double tj = xi[j];
      if (j < P) {
        const double zj = z[j];
        const double d = tj - zj;
        const double y = s * d;
        tj = tj + y;
        if constexpr (kBounds) {  // every j < P crosses; a snooker move is never reflected
          const bool below = tj < lo[j], above = tj > up[j];  // a NaN is neither
          n_left += below | above;
          if (bx.n_cross) {
            bx.n_cross[b * ld + j] += 1;
            if (below) bx.oob_lo[b * ld + j] += 1;
            if (above) bx.oob_hi[b * ld + j] += 1;
          }
        }
        oob |= !(tj >= lo[j] && tj <= up[j]);  // a NaN fails both comparisons
        const double f = tj - zj;
        const double ff = f * f;
        pE = pE + ff;
      }
      tr[j] = tj;
    }
    const double Dp = zs_sum64(pE);
    const double h = 0.5 * (double)(P - 1);
    const double l1 = log(Dp), l0 = log(D);
    const double dl = l1 - l0;
    lj = h * dl;
  } else {
    const int jrand = (int)zs_scale(w.z, (uint32_t)P);
    const double* x1 = Z + (int64_t)a * ld;
    const double* x2 = Z + (int64_t)c * ld;
    const double* jit = jitter + (int64_t)k * ld;
    // pass 1: the two uniforms of every coordinate; the crossing flags stay in the mask, the jitter uniform is parked
    uint64_t mask = 0;
    int it = 0;
    for (int j = lane; j < P; j += 64, ++it) {
      const uint4 v = rng(seed, key, gen, kPurposeCoord, i * 4096u + (uint32_t)j);
      const double u = u01(v.x, v.y);
      if (jump || u < CR || j == jrand) mask |= (uint64_t)1 << it;
      tr[j] = u01(v.z, v.w);
    }
    int dcross = __popcll(mask);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) dcross += __shfl_xor(dcross, d, 64);  // integers: the order does not matter
    const double gam = jump ? 1.0 : gamma0 / sqrt((double)(2 * dcross));
    // pass 2: lane l reads back the uniforms it parked at j = l, l + 64, ..
    it = 0;
    for (int64_t j = lane; j < ld; j += 64, ++it) {
      double tj = xi[j];
      uint8_t ob = 0;  // kBounds: the orientation bit of the trial's entry
      if constexpr (kBounds)
        if (bx.orient) ob = bx.orient[b * ld + j];
      if (j < P && ((mask >> it) & 1)) {
        const double v = tr[j];
        const double d = x1[j] - x2[j];
        double s = gam * d;
        if constexpr (kBounds)
          if (ob) s = -s;
        const double y = tj + s;
        const double e2 = 2.0 * v;
        const double f = e2 - 1.0;
        double zz = jit[j] * f;
        if constexpr (kBounds)
          if (ob) zz = -zz;
        tj = y + zz;
        if constexpr (kBounds) {
          const double lw = lo[j], uw = up[j];
          const bool below = tj < lw, above = tj > uw;  // of the raw trial; a NaN is neither
          n_left += below | above;
          if (bx.n_cross) {
            bx.n_cross[b * ld + j] += 1;
            if (below) bx.oob_lo[b * ld + j] += 1;
            if (above) bx.oob_hi[b * ld + j] += 1;
          }
          if (bx.reflect && (below | above)) {  // at most once: an overshoot beyond the width stays outside
            if (below) {
              const double e = lw - tj;
              tj = lw + e;
            } else {
              const double e = tj - uw;
              tj = uw - e;
            }
            ob ^= 1;
            n_refl += 1;
          }
        }
        oob |= !(tj >= lo[j] && tj <= up[j]);
      }
      tr[j] = tj;
      if constexpr (kBounds)
        if (bx.orient_t) bx.orient_t[b * ld + j] = ob;
    }
  }
  const bool out = __ballot(oob) != 0;  // wave-uniform
  double tot = qnan();
  if (!out) tot = prior_sum64(tr, mu + (int64_t)k * ld, sig + (int64_t)k * ld, P, lane);  // its own stores
  if (lane == 0) {
    pri[b] = tot;
    ljac[b] = out && snk ? qnan() : lj;
    move[b] = snk ? 1 : 0;
    active[b] = out ? 0 : 1;
  }
  if constexpr (kBounds) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {  // integers: the order does not matter
      n_left += __shfl_xor(n_left, d, 64);
      n_refl += __shfl_xor(n_refl, d, 64);
    }
    if (lane == 0) {  // a null move returned above: k_zs_decide reads neither for it
      bx.n_left_t[b] = n_left;
      bx.n_refl_t[b] = n_refl;
    }
  }
}

// kInit: s2 and the counters of every chain and, when keep_row >= 0, kept row 0. Else: the decisions of generation gen,
// then the archive rows (app_row >= 0: the cell's archive row that chain 0 goes to) and the kept row.
// kBounds (bx is read with it alone): the two per-proposal counts go to their logs, an evaluated proposal with a
// reflection is counted, and the trial's orientation row is copied with an accepted parallel trial.
template <bool kInit, bool kBounds, typename... Extra>
__global__ __launch_bounds__(kZsDecThreads) void k_zs_decide(
    const CellMeta* __restrict__ cells, const int32_t* __restrict__ cell_id, const int64_t* __restrict__ keys,
    const double* __restrict__ sigma2_0, const double* __restrict__ trial, const double* __restrict__ ss_t,
    const double* __restrict__ pri_t, const double* __restrict__ ljac, const uint8_t* __restrict__ move,
    const uint8_t* __restrict__ active, int n_pop, int64_t M_cap, int64_t ld, int64_t B, int64_t gen, uint64_t seed,
    int updatesigma, int64_t keep_row, int64_t app_row, int64_t log_row, double* pop, double* arch, double* ss, double* pri,
    double* s2, int32_t* __restrict__ n_acc, int32_t* __restrict__ n_oob, int32_t* __restrict__ n_null,
    double* __restrict__ chain, double* __restrict__ s2chain, double* __restrict__ sschain,
    double* __restrict__ prichain, double* __restrict__ logr, uint8_t* __restrict__ acc_log,
    uint8_t* __restrict__ oob_log, double* __restrict__ ljac_log, uint8_t* __restrict__ snk_log, Extra... extra) {
  static_assert(sizeof...(Extra) == (kBounds ? 1 : 0), "one ZsDecideBounds with kBounds, nothing without");
  const auto& bx = zs_extra(extra...);
  __shared__ uint8_t sh_take[kZsMaxPop];  // n_pop <= 4096 (the host checked)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t k = blockIdx.x;
  if (kInit) {
    const double s0 = sigma2_0[k];
    for (int i = threadIdx.x; i < n_pop; i += kZsDecThreads) {
      const int64_t b = k * n_pop + i;
      s2[b] = s0;
      n_acc[b] = 0;
      n_oob[b] = 0;
      n_null[b] = 0;
    }
  } else {
    const int64_t key = keys[k];
    const double shape = (double)cells[cell_id[k]].n;  // nobs / 2 with nobs = 2 N
    for (int i = threadIdx.x; i < n_pop; i += kZsDecThreads) {
      const int64_t b = k * n_pop + i;
      const bool act = active[b] != 0;
      const uint8_t mv = move[b];
      const double lj = ljac[b];
      const double s2i = s2[b];
      double ssi = ss[b], lr = qnan();
      bool take = false;
      if (act) {
        const double st = ss_t[b], pt = pri_t[b];
        const double qo = ssi / s2i;
        const double fo = qo + pri[b];  // formed afresh: s2 moves
        const double qn = st / s2i;
        const double fn = qn + pt;
        const double df = fn - fo;
        const double hl = -0.5 * df;
        lr = hl + lj;
        if (lr >= 0.0) {
          take = true;
        } else if (lr == lr) {  // a NaN logr rejects
          const uint4 r = rng(seed, key, gen, kPurposeAccept, (uint32_t)i);
          take = u01(r.x, r.y) < exp(lr);
        }
        if (take) {
          ss[b] = st;
          pri[b] = pt;
          ssi = st;
          n_acc[b] += 1;
        }
      } else if (mv == 2) {
        n_null[b] += 1;
      } else {
        n_oob[b] += 1;
      }
      if (updatesigma) {
        const double scale = 2.0 / ssi;
        const double g = gamma_unit_t(seed, key, gen, shape, kPurposeSigma, (uint32_t)i << 16);
        s2[b] = 1.0 / (g * scale);
      }
      sh_take[i] = take;
      if (log_row >= 0) {
        const int64_t at = log_row * B + b;
        if (logr) logr[at] = lr;
        if (acc_log) acc_log[at] = take;
        if (oob_log) oob_log[at] = act ? 0 : (mv == 2 ? 2 : 1);
        if (ljac_log) ljac_log[at] = lj;
        if (snk_log) snk_log[at] = mv != 0;
      }
      if constexpr (kBounds) {
        const int32_t nr = mv == 0 ? bx.n_refl_t[b] : 0;  // a null move's propose wrote neither count
        if (act && nr > 0) bx.n_reflected[b] += 1;
        if (log_row >= 0) {
          const int64_t at = log_row * B + b;
          if (bx.n_left_log) bx.n_left_log[at] = mv == 2 ? -1 : bx.n_left_t[b];
          if (bx.n_refl_log) bx.n_refl_log[at] = nr;
        }
      }
    }
    __syncthreads();
    for (int i = wave; i < n_pop; i += kZsDecWaves)
      if (sh_take[i]) {  // wave-uniform
        const int64_t b = k * n_pop + i;
        for (int64_t j = lane; j < ld; j += 64) pop[b * ld + j] = trial[b * ld + j];
        if constexpr (kBounds)
          if (bx.orient && move[b] == 0)  // a snooker move leaves the orientation as it is
            for (int64_t j = lane; j < ld; j += 64) bx.orient[b * ld + j] = bx.orient_t[b * ld + j];
      }
  }
  if (keep_row < 0 && app_row < 0) return;  // kernel arguments: the whole workgroup
  __syncthreads();
  // the rows and values stored above are this workgroup's own stores, ordered by the barrier
  for (int i = wave; i < n_pop; i += kZsDecWaves) {
    const int64_t b = k * n_pop + i;
    if (app_row >= 0) {
      double* to = arch + (k * M_cap + app_row + i) * ld;
      for (int64_t j = lane; j < ld; j += 64) to[j] = pop[b * ld + j];
    }
    if (keep_row >= 0) {
      const int64_t at = keep_row * B + b;
      for (int64_t j = lane; j < ld; j += 64) chain[at * ld + j] = pop[b * ld + j];
      if (lane == 0) {
        s2chain[at] = s2[b];
        sschain[at] = ss[b];
        prichain[at] = pri[b];
      }
    }
  }
}

int zs_sizes(int64_t n_sel, int64_t n_pop, int64_t M_g, int64_t M_cap, int64_t ld, int64_t gen) {
  if (n_sel < 1 || n_pop < 1 || n_pop > kZsMaxPop || ld < 1 || gen < 0) return TCI_EINVAL;
  if (gen > 0 && (M_g < 3 || M_g > M_cap || M_cap >= ((int64_t)1 << 24))) return TCI_EINVAL;
  if ((long double)n_sel * (long double)n_pop > 2147483647.0L) return TCI_ERANGE;
  return TCI_OK;
}

}  // namespace

}  // namespace tci

#endif  // TCI_DEMCZS_KERNELS_H_
