// tci_gamma.h -- the unit Gamma variate of the sigma2 update, shared by the sampler (tci_dram.hip) and the DE-MC
// population sampler (tci_demc.hip). Device code only.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

#include "tci_rng.h"

namespace tci {

constexpr uint32_t kPurposeGamma = 5;  // the sampler's P_GAMMA (tci_dram.hip)

// Gamma(a, 1) by Marsaglia & Tsang as the product d*v, for a >= 1: a = DramState::gshape = N/2 >= 2 on a plain chain
// and beta N/2 on a tempered rung, which dram_run_impl refuses below 1 (tci_dram_run_tempered); a Gamma(a, scale)
// variate is (d*v)*scale. The unit variate depends only on the stream and a, so the fused engine
// draws it ahead of the chain (k_draws) and the scale (2/SS of the current state) is applied when
// it is used: the same bits as gamma_at.
// Try `it` reads the calls base | it and base | it | 0x80000000 of stream (seed, c, step, purpose): base must leave
// the low 16 bits (it < 1024) and bit 31 alone. The defaults are the sampler's stream: base 0 is folded away, so its
// operations and bits are what they were.
template <int = 0>  // the body, inlined where the caller's register budget needs it (k_draws)
__device__ __forceinline__ double gamma_unit_t(uint64_t seed, int64_t c, int64_t step, double a,
                                               uint32_t purpose = kPurposeGamma, uint32_t base = 0) {
  const double d = a - 1.0 / 3.0, cc = 1.0 / sqrt(9.0 * d);
  for (uint32_t it = 0; it < 1024; ++it) {
    const uint4 r = rng(seed, c, step, purpose, base | it);
    const double u1 = u01(r.x, r.y), u2 = u01(r.z, r.w);
    const double x = sqrt(-2.0 * log(u1)) * cos(2.0 * M_PI * u2);
    const uint4 r2 = rng(seed, c, step, purpose, base | it | 0x80000000u);
    const double u = u01(r2.x, r2.y);
    double v = 1.0 + cc * x;
    if (v <= 0.0) continue;
    v = v * v * v;
    const double x2 = x * x;
    if (u < 1.0 - 0.0331 * x2 * x2) return d * v;  // squeeze (implies the log test)
    if (log(u) < 0.5 * x2 + d - d * v + d * log(v)) return d * v;
  }
  return a;  // unreachable in practice (acceptance > 0.95 per try)
}

}  // namespace tci
