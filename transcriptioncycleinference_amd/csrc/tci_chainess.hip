// tci_chainess.hip -- the multi-chain effective sample size of every group of replicate chains (BDA3 11.5, Geyer's
// initial monotone sequence), its autocorrelation time, its window and the pooled mean's Monte-Carlo standard error,
// reduced on the device; the definition is in include/tci.h.
//
// The moments (mu_j, s2_j of the whole chains and of their halves, the columns' states, pooled_std) are
// tci_chainrhat.hip's: launch_chainess runs launch_chainrhat first and reads its scratch, so both statistics see the
// same bits.
//
//   k_ce_lags   one workgroup (4 wavefronts) per (group, column tile, classic or split). A sequence is (chain, first
//               row, length): a whole chain (0, n) or a half (0, h) / (n - h, h). The lagged products are
//               tci_chain_dev.h's lag tile, as in k_cs_iact, with 0 past a sequence's end: the sum is linear, not
//               circular. A lag tile walks the group's sequences in order,
//               adding c_j(k) / L to a(k); rows past L - k0 have no partner at any lag of the tile and are not
//               read. After a lag tile wavefront 0 advances every column's pair sum (Geyer's P_i, Q_i); a column
//               that stopped is masked, and the workgroup ends with its last live column.
// A column with a non-finite entry in any chain of the group, a padding column and an empty group are written
// NaN / -1 before the lag loop and never enter it; their lanes issue no load. Chains of no group are in no
// group's list: nothing reads them. Every loop over lags is bounded by K = min(max_lag, L - 1).
//
// One lane sums c_j(k) over t = 0 .. L - 1 - k in increasing t with one FMA per product, whatever the tiles are, and
// the sequences are combined in order: an output's bits depend on the group's columns in chain order, on n and on
// max_lag alone.
#include <hip/hip_runtime.h>

#include <cmath>

#include "tci_chain_dev.h"
#include "tci_chainrhat_dev.h"
#include "tci_fp.h"
#include "tci_internal.h"

namespace tci {

namespace {

static_assert(kLagKT % 2 == 0, "a lag tile holds whole Geyer pairs");

struct CeMoments {
  const double *mu, *var;  // [kCrSeq][ncol]
  const int32_t* state;    // [ncol]
};

// out_d: [5][n_groups][ldc] = ess, ess_split, tau, tau_split, mcse; out_w: [2][n_groups][ldc].
__global__ __launch_bounds__(kChainThreads) void k_ce_lags(ChainView v, int64_t n, int64_t h, int64_t max_lag,
                                                           int tiles, int64_t n_groups,
                                                           const int32_t* __restrict__ g_off,
                                                           const int32_t* __restrict__ g_list, CeMoments mo,
                                                           const double* __restrict__ cap,
                                                           const double* __restrict__ rhat_out,
                                                           double* __restrict__ out_d, int32_t* __restrict__ out_w) {
  extern __shared__ __align__(16) double ce_lds[];
  __shared__ int s_live[kChainCols];
  __shared__ int s_any;
  double* A = ce_lds;                        // [kLagRT][64]: centred rows t0 ..
  double* B = ce_lds + kLagRT * kChainCols;  // [kLagBRows][64]: centred rows t0 + k0 ..; then a(k) [kLagKT][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int split = (int)(blockIdx.x & 1u);
  const int64_t gt = (int64_t)(blockIdx.x >> 1);
  const int64_t g = gt / tiles;
  const int64_t j = (gt % tiles) * kChainCols + lane;
  const int64_t ldc = v.ld + 1, ncol = v.n_chains * ldc, plane = n_groups * ldc;
  const int64_t id = g * ldc + j;
  const int32_t b = g_off[g];
  const int64_t M = g_off[g + 1] - b;
  const int nq = split ? 2 : 1, q0 = split ? 1 : 0;
  const int64_t L = split ? h : n, m = M * nq;
  const int64_t K = max_lag == 0 || max_lag > L - 1 ? L - 1 : max_lag;
  const int32_t* list = g_list + b;
  // the column's state: padding, a non-finite entry in a chain of the group and an empty group are done here
  bool ok = j < ldc && M > 0;
  if (ok) ok = chain_live(v, list[0], j);  // the group's chains have one npar (the host checked)
  for (int64_t k = 0; ok && k < M; ++k) ok = mo.state[(int64_t)list[k] * ldc + j] == COL_OK;
  bool live = ok && L >= 2;
  double W = 0.0, vplus = 0.0;
  if (live) {
    double sv, mb, dv;
    cr_between(CrSeqs{mo.mu, mo.var, list, ldc, ncol, j, q0, nq}, m, &sv, &mb, &dv);
    W = sv / (double)m;
    const double T = m >= 2 ? dv / (double)(m - 1) : 0.0;
    vplus = ((double)(L - 1) / (double)L) * W + T;
  } else if (wave == 0 && j < ldc) {
    out_d[split * plane + id] = qnan();
    out_d[(2 + split) * plane + id] = qnan();
    if (!split) out_d[4 * plane + id] = qnan();
    out_w[split * plane + id] = ok ? 0 : -1;  // L < 2: a column, with no lag to sum
  }
  bool any = __ballot(live) != 0;  // every wavefront holds the same 64 columns: the same answer in all four
  // Geyer's running state (wavefront 0)
  double Q = 0.0, sum = 0.0;
  for (int64_t k0 = 0; any && k0 <= K; k0 += kLagKT) {
    double a_k[kLagLW];
#pragma unroll
    for (int k = 0; k < kLagLW; ++k) a_k[k] = 0.0;
    for (int64_t sq = 0; sq < m; ++sq) {
      const int64_t c = list[sq / nq];
      const int64_t r0 = split && (sq & 1) ? n - h : 0;
      const double muj = live ? mo.mu[(int64_t)(q0 + (int)(sq % nq)) * ncol + c * ldc + j] : 0.0;
      const ChainCol col = chain_col(v, c, j, live);
      const double* seq = live ? col.ptr + r0 * col.rs : nullptr;
      // row t of the sequence, centred; 0 past its end: the sum is linear, not circular
      auto y = [&](int64_t t) { return live && t < L ? seq[t * col.rs] - muj : 0.0; };
      double acc[kLagLW];
#pragma unroll
      for (int k = 0; k < kLagLW; ++k) acc[k] = 0.0;
      for (int64_t t0 = 0; t0 < L - k0; t0 += kLagRT)  // a row t >= L - k0 has no partner t + k < L, k >= k0
        lag_tile(A, B, lane, wave, live, t0, t0 + k0, y, y, acc);
#pragma unroll
      for (int k = 0; k < kLagLW; ++k) a_k[k] += acc[k] / (double)L;
    }
#pragma unroll
    for (int k = 0; k < kLagLW; ++k) a_k[k] = a_k[k] / (double)m;
    lag_hand(B, lane, wave, live, a_k);
    if (wave == 0) {
      if (live) {
        bool fin = false, stopped = false;
        int64_t s = 0;
        for (int ii = 0; ii < kLagKT / 2; ++ii) {
          const int64_t i = k0 / 2 + ii;
          if (2 * i + 1 > K) {  // the pairs ran out
            s = i;
            fin = true;
            break;
          }
          const double ae = B[(2 * ii) * kChainCols + lane], ao = B[(2 * ii + 1) * kChainCols + lane];
          const double re = i == 0 ? 1.0 : 1.0 - (W - ae) / vplus;
          const double ro = 1.0 - (W - ao) / vplus;
          const double P = re + ro;
          if (i == 0) {
            Q = P;
            sum = P;
            continue;
          }
          if (!(P > 0.0)) {  // a NaN stops
            s = i;
            fin = stopped = true;
            break;
          }
          Q = P < Q ? P : Q;  // a NaN Q_0 stays
          sum += Q;
        }
        if (!fin && k0 + kLagKT + 1 > K) {  // the next tile's first pair is past K
          s = k0 / 2 + kLagKT / 2;
          fin = true;
        }
        if (fin) {
          const bool capped = !stopped && K < L - 1;
          const double tau = capped ? pinf() : -1.0 + 2.0 * sum;
          const double cp = cap[split * n_groups + g];
          const double q = (double)(m * L) / tau;
          const double ess = tau != tau ? qnan() : tau > 0.0 ? (q < cp ? q : cp) : cp;
          out_d[split * plane + id] = ess;
          out_d[(2 + split) * plane + id] = tau;
          if (!split) out_d[4 * plane + id] = rhat_out[3 * plane + id] / sqrt(ess);
          out_w[split * plane + id] = (int32_t)(2 * s);
          live = false;
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

int launch_chainess(const double* chain, const double* s2, int64_t n_rows, int64_t n_chains, int64_t ld,
                    const int32_t* npar, const int32_t* group, int64_t n_groups, const int32_t* g_off,
                    const int32_t* g_list, int64_t max_lag, const double* cap, void* scratch, double* rhat_out,
                    double* out_d, int32_t* out_w, void* stream) {
  if (!cap || !rhat_out || !out_d || !out_w || max_lag < 0) return TCI_EINVAL;
  int rc = launch_chainrhat(chain, s2, n_rows, n_chains, ld, npar, group, n_groups, g_off, g_list, scratch, rhat_out,
                            stream);
  if (rc != TCI_OK) return rc;
  CeMoments mo;
  rc = chainrhat_scratch_moments(scratch, n_rows, n_chains, ld, n_groups, &mo.mu, &mo.var, &mo.state);
  if (rc != TCI_OK) return rc;
  const int64_t tiles = (ld + 1 + kChainCols - 1) / kChainCols;
  if ((long double)n_groups * tiles * 2 > 2147483647.0L) return TCI_ERANGE;
  if (ensure_dyn_lds((const void*)k_ce_lags, kLagLds) != TCI_OK) return TCI_EHIP;
  const ChainView v{chain, s2, npar, n_chains, ld};
  hipLaunchKernelGGL(k_ce_lags, dim3((unsigned)(n_groups * tiles * 2)), dim3(kChainThreads), kLagLds,
                     (hipStream_t)stream, v, n_rows, n_rows / 2, max_lag, (int)tiles, n_groups, g_off, g_list, mo, cap,
                     rhat_out, out_d, out_w);
  return hipGetLastError() == hipSuccess ? TCI_OK : TCI_EHIP;
}

}  // namespace tci
