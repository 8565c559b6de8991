// The integer half of the base-noise generator: Philox4x32-10 (Salmon et al. 2011, "Parallel random numbers: as
// easy as 1, 2, 3") and the map of one output word to a uniform in (0, 1].  __host__ __device__, so the CPU
// test-suite checks the very code the kernels run (hostcheck.cpp) against an independent reference
// (tests/philox_ref.py) and the paper's known-answer vectors.  Box-Muller on the hardware transcendentals
// (box_muller4) is device-only and stays in common.hpp.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VISSM_HD __host__ __device__
#else
#define VISSM_HD
#ifndef __forceinline__
#define __forceinline__ inline __attribute__((always_inline))
#endif
#endif

namespace vissm {

// ---------------------------------------------------------------------------
// Philox4x32-10, counter = (lo(ctr), hi(ctr), lo(sub), hi(sub)), key = seed.
// ---------------------------------------------------------------------------
struct u4 { uint32_t x, y, z, w; };

VISSM_HD __forceinline__ u4 philox4x32_10(u4 c, uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
  const uint32_t W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    // one 32x32 -> 64-bit product per word (v_mad_u64_u32) instead of separate hi / lo multiplies
    const uint64_t p0 = static_cast<uint64_t>(M0) * c.x, p1 = static_cast<uint64_t>(M1) * c.z;
    const uint32_t hi0 = static_cast<uint32_t>(p0 >> 32), lo0 = static_cast<uint32_t>(p0);
    const uint32_t hi1 = static_cast<uint32_t>(p1 >> 32), lo1 = static_cast<uint32_t>(p1);
    u4 n;
    n.x = hi1 ^ c.y ^ k0;
    n.y = lo1;
    n.z = hi0 ^ c.w ^ k1;
    n.w = lo0;
    c = n;
    k0 += W0;
    k1 += W1;
  }
  return c;
}

VISSM_HD __forceinline__ float u01(uint32_t x) {
  // (0, 1]: never 0 so log() is finite
  return (static_cast<float>(x >> 8) + 1.0f) * (1.0f / 16777216.0f);
}

}  // namespace vissm
