// Shared math of the bootstrap particle filter (particle.hip; include/vissm.h vissm_particle_filter): the
// observation log-weight, its integer quantisation, the log-evidence increment, the effective sample size and
// systematic resampling in integers.  __host__ __device__, so the CPU test-suite checks the very code the kernel runs
// (hostcheck.cpp) against Python big-int arithmetic.
//
// Everything after the fp32 exp is integer: q_i = trunc(exp(logw_i - m) 2^40) with m the maximum over the live
// particles (a maximum is exact in any order; the scale is a power of two, so the product is exact), W = sum q_i an
// exact integer below 2^50 for N <= 1024, C the inclusive cumulative sum.  With a 24-bit integer U the thresholds
//   tau_j = ((j 2^24 + U) W) >> (24 + log2 N)
// are those of systematic resampling at u = U 2^-24: anc[j] = #{i : C_i <= tau_j} <= N - 1 because tau_j < W.
// The result depends on no summation order, launch geometry or block schedule, so a test reproduces it exactly.
#pragma once
#include <stdint.h>

#include "sim_math.hpp"
#include "rng_math.hpp"

namespace vissm {
namespace pf {

constexpr int kScaleBits = 40;                       // q = trunc(w 2^40)
constexpr int kUBits = 24;                           // the resampling integer U < 2^24
constexpr double kScaleLn = 27.725887222397812;      // 40 ln 2
constexpr int kMinN = 64, kMaxN = 1024;

// N in {64, 128, 256, 512, 1024}: one particle per lane, a power of two (the thresholds shift, never divide)
VHD bool valid_n(int n) { return n >= kMinN && n <= kMaxN && (n & (n - 1)) == 0; }

VHD constexpr int log2_of(int n) {
  int l = 0;
  while ((1 << l) < n) ++l;
  return l;
}

// log-weight of a live particle: sum over the observed coordinates of log N(y_d; x_d, sd) (em::obs_term); a
// coordinate with bin = 0 is not read (its y may be any filler)
VHD float obs_logw(int S, const float* x, const float* y, const float* bin, float sd) {
  float lw = 0.f;
  for (int d = 0; d < S; ++d) {
    if (bin[d] != 0.f) {
      float gx;
      lw += em::obs_term(x[d], y[d], bin[d], sd, &gx);
    }
  }
  return lw;
}

// q = trunc(exp(logw - m) 2^40), exp in fp32; 0 for a dead particle and where logw - m is not a number (m = -inf:
// no live particle has a finite weight)
VHD uint64_t quantise(float logw, float m, bool alive) {
  if (!alive) return 0u;
  const float v = VEXP(logw - m) * 0x1.0p40f;
  return v >= 0.f ? static_cast<uint64_t>(v) : 0u;
}

// high and low words of a 64 x 64 -> 128-bit product
VHD void mul64(uint64_t a, uint64_t b, uint64_t* hi, uint64_t* lo) {
#if defined(__HIP_DEVICE_COMPILE__)
  *hi = __umul64hi(a, b);
  *lo = a * b;
#else
  const unsigned __int128 p = static_cast<unsigned __int128>(a) * b;
  *hi = static_cast<uint64_t>(p >> 64);
  *lo = static_cast<uint64_t>(p);
#endif
}

// tau_j = ((j 2^24 + U) W) >> (24 + log2 N); j < N <= 2^10, U < 2^24, W < 2^50: the product stays below 2^84 and
// tau_j below W
VHD uint64_t threshold(uint32_t j, uint32_t U, uint64_t W, int log2n) {
  const uint64_t a = (static_cast<uint64_t>(j) << kUBits) | U;
  uint64_t hi, lo;
  mul64(a, W, &hi, &lo);
  const int s = kUBits + log2n;  // 30 .. 34
  return (hi << (64 - s)) | (lo >> s);
}

// #{i : C_i <= tau} of a non-decreasing C[0 .. n): binary search
VHD int ancestor(const uint64_t* C, int n, uint64_t tau) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (C[mid] <= tau) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// log p(y_t | y_<t) estimate: m + log W - 40 ln 2 - ln N (W > 0)
VHD double ll_increment(float m, uint64_t W, int n) {
#if defined(__HIP_DEVICE_COMPILE__)
  return static_cast<double>(m) + ::log(static_cast<double>(W)) - kScaleLn - ::log(static_cast<double>(n));
#else
  return static_cast<double>(m) + std::log(static_cast<double>(W)) - kScaleLn - std::log(static_cast<double>(n));
#endif
}

// W^2 / sum q_i^2
VHD double ess(uint64_t W, double sum_q2) {
  const double w = static_cast<double>(W);
  return w * w / sum_q2;
}

// the resampling integer of the filter whose first Philox row is r, at absolute step t: the first word's top 24 bits
// of counter (t, 1, lo32(r), hi32(r)).  The normals' counters carry 0 in their second word, so the two never meet.
VHD uint32_t resample_u(uint64_t seed, uint32_t t, uint64_t r) {
  const u4 c{t, 1u, static_cast<uint32_t>(r), static_cast<uint32_t>(r >> 32)};
  return philox4x32_10(c, static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32)).x >> 8;
}

// serial systematic resampling (host checks): anc[j] for j < n from the weights q; returns W (0: anc untouched)
inline uint64_t resample(const uint64_t* q, int n, uint32_t U, int32_t* anc, uint64_t* C) {
  uint64_t W = 0;
  for (int i = 0; i < n; ++i) C[i] = (W += q[i]);
  if (W == 0) return 0;
  const int l = log2_of(n);
  for (int j = 0; j < n; ++j) anc[j] = ancestor(C, n, threshold(static_cast<uint32_t>(j), U, W, l));
  return W;
}

}  // namespace pf
}  // namespace vissm
