// tci_fp.h -- the special doubles the kernels write and the finiteness test they share: one spelling of each, so
// every "no value" in an output is the same quiet NaN.
#pragma once

#include <hip/hip_runtime.h>

namespace tci {

__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7FF8000000000000ll); }
__device__ __forceinline__ double pinf() { return __longlong_as_double(0x7FF0000000000000ll); }

// x - x is 0 for a finite x and NaN for NaN and +-Inf: the library is built without any fast-math flag (build.py),
// so the compiler may not fold it.
__device__ __forceinline__ bool is_finite(double x) { return (x - x) == 0.0; }

}  // namespace tci
