// tci_key.h -- the 64-bit total order on doubles the quantile kernels select and sort by.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace tci {

constexpr uint64_t kSign = 0x8000000000000000ull;

// NaNs canonicalised to one positive quiet NaN, then the sign-flip map (negative: all bits inverted; else: sign
// bit set): -Inf < ... < -0 < +0 < ... < +Inf < NaN as unsigned integers.
__device__ __forceinline__ uint64_t to_key(double x) {
  uint64_t u = (uint64_t)__double_as_longlong(x);
  if (x != x) u = 0x7FF8000000000000ull;
  return (u & kSign) ? ~u : (u | kSign);
}

__device__ __forceinline__ double from_key(uint64_t k) {
  return __longlong_as_double((long long)((k & kSign) ? (k ^ kSign) : ~k));
}

}  // namespace tci
