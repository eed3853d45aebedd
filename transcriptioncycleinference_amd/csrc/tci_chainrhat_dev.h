// tci_chainrhat_dev.h -- what the reductions across chains share (tci_chainrhat.hip, tci_chainess.hip): the scratch
// of the per-sequence moments and the between/within combination of a group's sequences. Both
// files take mu_j, s2_j, W, mubar and T from here, so both see the same bits.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tci {

namespace {

constexpr int kCrSeq = 3;  // sequences per chain column: whole, half A, half B

// The scratch of one call, carved from one allocation (8-byte items first).
struct CrScratch {
  double *p_s, *p_c;  // [S][kCrSeq][ncol] compensated sums (pass 1); p_s again: centred squares (pass 2)
  double* mu;         // [kCrSeq][ncol]
  double* var;        // [kCrSeq][ncol]
  uint32_t* p_f;      // [S][ncol] flags
  int32_t* state;     // [ncol] COL_PAD / COL_OK / COL_BAD (tci_chain_dev.h)
};

// The m sequences of one group column, in order: sequence k is sequence q0 + k % nq of the group's chain k / nq.
struct CrSeqs {
  const double *mu, *var;  // CrScratch's
  const int32_t* list;     // the group's chains
  int64_t ldc, ncol, j;
  int q0, nq;
  __device__ __forceinline__ int64_t at(int64_t k) const {
    return (int64_t)(q0 + (int)(k % nq)) * ncol + (int64_t)list[k / nq] * ldc + j;
  }
};

// sum_v = sum_k s2_k, mubar and dev = sum_k (mu_k - mubar)^2 of the sequences; equal means: mubar is their value.
__device__ __forceinline__ void cr_between(const CrSeqs& q, int64_t m, double* sum_v, double* mubar, double* dev) {
  double sv = 0.0, sm = 0.0;
  const double first = q.mu[q.at(0)];
  bool same = true;
  for (int64_t k = 0; k < m; ++k) {
    const double mu = q.mu[q.at(k)];
    sv += q.var[q.at(k)];
    sm += mu;
    same &= mu == first;
  }
  const double mb = same ? first : sm / (double)m;
  double dv = 0.0;
  for (int64_t k = 0; k < m; ++k) {
    const double d = q.mu[q.at(k)] - mb;
    dv += d * d;
  }
  *sum_v = sv;
  *mubar = mb;
  *dev = dv;
}

}  // namespace

}  // namespace tci
