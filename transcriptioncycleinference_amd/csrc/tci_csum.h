// tci_csum.h -- the compensated column sum shared by the chain reductions: every one of them takes a column's
// mean from it, so all centre a column on the same bits.
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
  // another sum's (s, c) joins this one: its s as one more term, its compensation as it is
  __device__ __forceinline__ void merge(double s2, double c2) {
    add(s2);
    c += c2;
  }
  __device__ __forceinline__ double total() const { return s + c; }
};

}  // namespace tci
