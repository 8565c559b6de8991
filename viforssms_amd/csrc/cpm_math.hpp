// Shared math of the correlated pseudo-marginal chain of the stochastic-volatility model (sv_sorted.hip; include/vissm.h
// vissm_sv_filter_sorted, vissm_sv_cpmmh; Deligiannidis, Doucet & Pitt 2018): the autoregressive move of the filter's
// carried normals, the sort key of a particle and the resampling integer of a carried normal.  __host__ __device__, so
// the CPU test-suite checks the very code the kernels run (hostcheck.cpp) against numpy.
//
//   cn(u, eps, rho, sigma) = fl32(fl32(rho u) + fl32(sigma eps)): the Crank-Nicolson move u' = rho u + sqrt(1 - rho^2) eps,
//              which leaves N(0, 1) invariant; the two products are rounded on their own (no contraction), so numpy
//              float32 reproduces it bit for bit
//   sigma_of(rho) = float(sqrt(1 - (double) rho (double) rho)), once on the host side of the entry
//   sort_key(h)   the fp32 bits as a uint32 whose unsigned order is the numeric order: b ^ 0x80000000 for a clear sign
//              bit, ~b for a set one (-0 before +0); anything not finite -> 0xFFFFFFFF, so a dead particle sorts last.
//              key_value is its inverse (0xFFFFFFFF -> the canonical quiet NaN).  Equal keys are equal states, so the
//              sorted array is unique whatever a sort does with ties.
//   resample_u(ur) = min(2^24 - 1, (uint32) floor(Phi(ur) 2^24)), Phi(x) = 1/2 erfc(-x / sqrt 2) in double: the carried
//              normal as the 24-bit integer pf::threshold takes
#pragma once
#include <math.h>
#include <stdint.h>

#include "rng_math.hpp"

namespace vissm {
namespace cpm {

// a product that must not be fused with the sum it feeds (mh::unfused, for a float)
VISSM_HD inline float unfused(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(x));
#else
  asm volatile("" : "+m"(x));
#endif
  return x;
}

VISSM_HD inline float cn(float u, float eps, float rho, float sigma) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float a = unfused(rho * u), b = unfused(sigma * eps);
  return a + b;
}

inline float sigma_of(float rho) {
  const double r = static_cast<double>(rho);
  return static_cast<float>(::sqrt(1.0 - r * r));
}

// rho in [0, 1): a NaN fails both comparisons
inline bool valid_rho(float rho) { return rho >= 0.f && rho < 1.f; }

constexpr uint32_t kDeadKey = 0xFFFFFFFFu;

VISSM_HD inline uint32_t sort_key(float h) {
  const uint32_t b = __builtin_bit_cast(uint32_t, h);
  if ((b & 0x7F800000u) == 0x7F800000u) return kDeadKey;  // inf or NaN
  return (b & 0x80000000u) ? ~b : b ^ 0x80000000u;
}

VISSM_HD inline float key_value(uint32_t k) {
  if (k == kDeadKey) return __builtin_nanf("");
  return __builtin_bit_cast(float, (k & 0x80000000u) ? k ^ 0x80000000u : ~k);
}

VISSM_HD inline uint32_t resample_u(float ur) {
  const double p = 0.5 * ::erfc(-static_cast<double>(ur) * 0.70710678118654752440);
  const double s = ::floor(p * 16777216.0);
  if (!(s >= 0.0)) return 0u;  // (a NaN: never from finite aux)
  return s >= 16777215.0 ? 16777215u : static_cast<uint32_t>(s);
}

}  // namespace cpm
}  // namespace vissm
