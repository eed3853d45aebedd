// tci_csum.h -- the compensated column sum shared by the chain reductions (tci_chainstats.hip,
// tci_chaincov.hip): both take a column's mean from it, so both centre a column on the same bits.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

namespace tci {

// Neumaier's compensated sum: the means are right to the last bit or two whatever n is.
struct CSum {
  double s = 0.0, c = 0.0;
  __device__ __forceinline__ void add(double x) {
    const double t = s + x;
    c += fabs(s) >= fabs(x) ? (s - t) + x : (x - t) + s;
    s = t;
  }
  __device__ __forceinline__ double total() const { return s + c; }
};

}  // namespace tci
