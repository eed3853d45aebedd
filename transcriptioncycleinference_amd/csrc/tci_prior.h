// tci_prior.h -- the Gaussian prior sum of one theta row in the order include/tci.h fixes for tci_chainlp's pri_t,
// shared by tci_chainlp.hip and tci_modesearch.hip. Device code only.
#pragma once

#include <hip/hip_runtime.h>

namespace tci {

// SUM_{j < P} ((th_j - m_j) / sg_j)^2 by one wavefront, every lane calling with its lane index: lane l sums the terms
// j = l, l + 64, .. in ascending j from 0.0, the 64 partials are added in ascending lane order from 0.0 by every lane
// alike. A term with sg_j = +Inf is exactly 0. Entries j >= P are never read.
__device__ __forceinline__ double prior_sum64(const double* th, const double* m, const double* sg, int P, int lane) {
  double part = 0.0;
  for (int j = lane; j < P; j += 64) {
    const double d = th[j] - m[j];
    const double q = d / sg[j];
    part += q * q;
  }
  double tot = 0.0;
#pragma unroll
  for (int l = 0; l < 64; ++l) tot += __shfl(part, l, 64);
  return tot;
}

}  // namespace tci
