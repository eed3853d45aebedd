// tci_rng.h -- the counter-based generator of the sampler (tci_dram.hip) and of the mode search (tci_modesearch.hip):
// Philox4x32-10 keyed by (seed), counter (chain, step, purpose, index). A stream is reproducible and independent of
// launch geometry. Purposes 1-6 are the sampler's (tci_dram.hip), 7 and 8 the mode search's, 9-12 the DE-MC sampler's
// (tci_demc.hip), 13-16 the DE-MC(zs) sampler's (tci_demczs.hip). Device code only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tci {

// The 32 x 32 -> 64-bit product of a Philox round in one v_mad_u64_u32: the compiler's
// v_mul_lo_u32 + v_mul_hi_u32 pair is two quarter-rate instructions (draws pass: TestData 105.0 ->
// 97.5 us per chunk, config 4 62.1 -> 52.7 ms per 1,000 steps, r03v; the same exact product).
__device__ __forceinline__ uint64_t mul64(uint32_t a, uint32_t b) {
  uint64_t r, carry;
  asm("v_mad_u64_u32 %0, %1, %2, %3, 0" : "=v"(r), "=s"(carry) : "v"(a), "v"(b));
  return r;
}

// Philox4x32-10 (Salmon et al. 2011).
__device__ __forceinline__ uint4 philox(uint4 c, uint2 k) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = mul64(0xD2511F53u, c.x), p1 = mul64(0xCD9E8D57u, c.z);
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
    const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    c = make_uint4(__builtin_amdgcn_bitop3_b32(hi1, c.y, k.x, 0x96), lo1, __builtin_amdgcn_bitop3_b32(hi0, c.w, k.y, 0x96),
                   lo0);  // 0x96: three-input xor
    k.x += 0x9E3779B9u;
    k.y += 0xBB67AE85u;
  }
  return c;
}

__device__ __forceinline__ uint4 rng(uint64_t seed, int64_t chain, int64_t step, uint32_t purpose, uint32_t idx) {
  const uint4 ctr = make_uint4((uint32_t)chain, (uint32_t)step, ((uint32_t)(step >> 32) & 0x00FFFFFFu) | (purpose << 24),
                               idx);
  return philox(ctr, make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
}

// Uniform in (0,1) from 64 random bits (53-bit mantissa, never 0 or 1).
__device__ __forceinline__ double u01(uint32_t a, uint32_t b) {
  const uint64_t x = (((uint64_t)a << 32) | b) >> 11;
  return ((double)x + 0.5) * 0x1p-53;
}

}  // namespace tci
