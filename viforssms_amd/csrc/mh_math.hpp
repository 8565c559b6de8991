// Shared math of particle marginal Metropolis-Hastings (pmmh.hip; include/vissm.h vissm_pmmh): the Philox words of an
// iteration's proposal, the uniform of its decision, the random-walk proposal, the Gaussian log-prior and the
// acceptance rule.  __host__ __device__, so the CPU test-suite checks the very code the kernel runs (hostcheck.cpp)
// against numpy.
//
// Iteration i of chain c of C, N particles, first row row0:  r = row0 + (i C + c) N, the first Philox row of the
// iteration's filter.  Counter (g, 2, lo32(r), hi32(r)) under the key: the second word 2 keeps these clear of the
// filter's normals (0) and resampling integers (1) on the same row.
//   g = 0, 1   Box-Muller on the four words -> xi_0 .. xi_7, of which the first P are used
//   g = 2      first word x -> u = ((x >> 8) + 1/2) 2^-24 in (0, 1), exact in double
//   theta'_p = float(theta_p + sum_{j <= p} L_pj xi_j): double, ascending j (a product of two floats is exact in
//              double, so a fused multiply-add gives the same bits)
//   lp = -1/2 sum_p ((theta_p - m_p) / s_p)^2: double, ascending p, no contraction (the pragma below), so numpy's
//              subtract / divide / multiply / add reproduce it exactly
//   accept iff log(u) < (ll' - ll) + (lp' - lp), in double, in this arrangement: a dead proposal (ll' = -inf) gives
//              -inf and is rejected, a chain at ll = -inf accepts any finite proposal (+inf), and -inf against -inf gives
//              NaN, which compares false: rejected.
// The device's Box-Muller is box_muller4 (common.hpp, the hardware transcendentals every stream of the library uses);
// box_muller4_ref below is the same formula in double rounded to fp32, for the host checks and replays.
#pragma once
#include <math.h>
#include <stdint.h>

#include "rng_math.hpp"

namespace vissm {
namespace mh {

constexpr int kMaxP = 5;       // theta length: VISSM_MODEL_P
constexpr uint32_t kWord1 = 2u;  // the second counter word of the proposal's and the decision's Philox blocks

// the first Philox row of iteration i of chain c (uint64 arithmetic wraps as the rows of every stream do)
VISSM_HD inline uint64_t row_of(uint64_t row0, uint64_t i, uint64_t C, uint64_t c, uint64_t N) {
  return row0 + (i * C + c) * N;
}

VISSM_HD inline u4 words(uint32_t g, uint64_t r, uint64_t seed) {
  const u4 c{g, kWord1, static_cast<uint32_t>(r), static_cast<uint32_t>(r >> 32)};
  return philox4x32_10(c, static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32));
}

// u = ((x >> 8) + 1/2) 2^-24: never 0 or 1
VISSM_HD inline double uniform(uint32_t x) { return (static_cast<double>(x >> 8) + 0.5) * 0x1.0p-24; }

VISSM_HD inline double log_uniform(uint32_t x) { return ::log(uniform(x)); }

// theta' from theta, the lower factor L [P][P] and the normals xi[0 .. P)
VISSM_HD inline void propose(const float* th, const float* L, const float* xi, int P, float* out) {
#pragma unroll
  for (int p = 0; p < P; ++p) {
    double s = static_cast<double>(th[p]);
#pragma unroll
    for (int j = 0; j <= p; ++j) s += static_cast<double>(L[p * P + j]) * static_cast<double>(xi[j]);
    out[p] = static_cast<float>(s);
  }
}

// prior [P][2] = (mean, sd)
VISSM_HD inline double log_prior(const float* th, const float* prior, int P) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double acc = 0.0;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const double z = (static_cast<double>(th[p]) - static_cast<double>(prior[2 * p])) /
                     static_cast<double>(prior[2 * p + 1]);
    const double zz = z * z;
    acc = acc + zz;
  }
  return -0.5 * acc;
}

VISSM_HD inline bool accept(double logu, double ll_prop, double ll_cur, double lp_prop, double lp_cur) {
  return logu < (ll_prop - ll_cur) + (lp_prop - lp_cur);
}

// Box-Muller on one Philox block in double, rounded to fp32: common.hpp's box_muller4 without the hardware
// transcendentals (host checks and replays only)
inline void box_muller4_ref(u4 r, float* v) {
  const double kTwoPi = 6.283185307179586476925286766559;
  const double r1 = ::sqrt(-2.0 * ::log(static_cast<double>(u01(r.x))));
  const double r2 = ::sqrt(-2.0 * ::log(static_cast<double>(u01(r.z))));
  const double a1 = kTwoPi * static_cast<double>(u01(r.y)), a2 = kTwoPi * static_cast<double>(u01(r.w));
  v[0] = static_cast<float>(r1 * ::cos(a1));
  v[1] = static_cast<float>(r1 * ::sin(a1));
  v[2] = static_cast<float>(r2 * ::cos(a2));
  v[3] = static_cast<float>(r2 * ::sin(a2));
}

}  // namespace mh
}  // namespace vissm
