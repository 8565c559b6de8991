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

// ---- the adaptive chain (vissm_pmmh_adaptive): robust adaptive Metropolis (Vihola 2012) -----------------------------
// While the absolute iteration i is below adapt_end the chain's own factor follows
//   L' L'^T = L (I + d xi xi^T / |xi|^2) L^T,   d = eta (alpha - target),   eta = min(1, P (i + 1)^-gamma)
// by a rank-one Cholesky update (d > 0) or downdate (d < 0) of L, with alpha the acceptance probability of the
// iteration's proposal and xi its first P normals.  |d| < 1, so the product is positive definite; the factor is kept
// in fp32 (propose() reads it as before) and an update that cannot be represented leaves it as it was.

// e^x for x <= 0 and log(n) for n >= 1, to a few units of 1e-16 relative.  The kernel does not call the device
// library's exp and pow here: their polynomials' twenty-odd double constants are hoisted out of the iteration loop into
// vector registers, where they stay live over the filter loop, and the 1024-lane FHN block spills.  These keep their
// coefficients in a table that the rolled Horner loops read entry by entry (uniform addresses: scalar loads).
//   exp: k = rint(x log2 e), f = x - k ln 2 (ln 2 split in two, |f| <= 0.347), the Taylor series to f^14 (the next term
//        is below 1e-19), scaled by 2^k; 0 below -745.5, where e^x rounds to 0
//   log: n = m 2^e with m in [sqrt(1/2), sqrt 2), s = (m - 1) / (m + 1), log m = 2 s sum_{j <= 10} s^2j / (2 j + 1)
//        (|s| <= 0.172: the next term is below 1e-18), plus e ln 2
constexpr double kLn2Hi = 6.93147180369123816490e-01, kLn2Lo = 1.90821492927058770002e-10;

VISSM_HD inline double exp_nonpos(double x) {
  static constexpr double c[15] = {1.0, 1.0, 0.5, 0.16666666666666666, 0.041666666666666664, 0.008333333333333333,
                                   0.001388888888888889, 0.0001984126984126984, 2.48015873015873e-05,
                                   2.7557319223985893e-06, 2.755731922398589e-07, 2.505210838544172e-08,
                                   2.08767569878681e-09, 1.6059043836821613e-10, 1.1470745597729725e-11};
  if (!(x > -745.5)) return 0.0;
  const double k = ::rint(x * 1.4426950408889634);
  const double f = (x - k * kLn2Hi) - k * kLn2Lo;
  double p = c[14];
#pragma unroll 1
  for (int j = 13; j >= 0; --j) p = p * f + c[j];
  return ::ldexp(p, static_cast<int>(k));
}

VISSM_HD inline double log_pos(double n) {
  static constexpr double c[11] = {1.0, 0.3333333333333333, 0.2, 0.14285714285714285, 0.1111111111111111,
                                   0.09090909090909091, 0.07692307692307693, 0.06666666666666667, 0.058823529411764705,
                                   0.05263157894736842, 0.047619047619047616};
  int e = 0;
  double m = ::frexp(n, &e);
  if (m < 0.70710678118654752) {
    m = 2.0 * m;
    e = e - 1;
  }
  const double s = (m - 1.0) / (m + 1.0), z = s * s;
  double p = c[10];
#pragma unroll 1
  for (int j = 9; j >= 0; --j) p = p * z + c[j];
  const double ed = static_cast<double>(e);
  return ed * kLn2Hi + (ed * kLn2Lo + 2.0 * s * p);
}

// min(1, exp((ll' - ll) + (lp' - lp))) from the state before the decision: accept()'s expression.  NaN -> 0 (-inf
// against -inf), a dead proposal -> 0, a chain at -inf meeting a finite proposal -> 1.
VISSM_HD inline double accept_prob(double ll_prop, double ll_cur, double lp_prop, double lp_cur) {
  const double r = (ll_prop - ll_cur) + (lp_prop - lp_cur);
  if (r != r) return 0.0;
  return r >= 0.0 ? 1.0 : exp_nonpos(r);
}

// the step size of the absolute iteration i: min(1, P (i + 1)^-gamma)
VISSM_HD inline double adapt_eta(int P, int64_t i, double gamma) {
  const double e = static_cast<double>(P) * exp_nonpos(-gamma * log_pos(static_cast<double>(i + 1)));
  return e < 1.0 ? e : 1.0;
}

// A product that must not be fused with the sum it feeds.  The library is built with -ffp-contract=fast, which fuses in
// the backend whatever a contract(off) pragma says; the device's result then differs from numpy's in the last bit.
VISSM_HD inline double unfused(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(x));
#endif
  return x;
}

// L [P][P] (lower; the strict upper part is neither read nor written) -> L' in place.  Double throughout, in the
// order written and without contraction, so numpy's multiply / add / divide / sqrt reproduce it exactly; every entry is
// rounded to fp32 at the end.  Returns false and leaves L as it was when there is nothing to do (xi = 0, d = 0 or not
// finite) or the pass breaks down (a diagonal that is not positive, before or after rounding; an entry that is not
// finite).  work [adapt_work(P)] doubles holds the copy of L, v and xi: the kernel passes LDS and the loops stay
// rolled, so the update costs its one thread a handful of registers and no scratch.
VISSM_HD constexpr int adapt_work(int P) { return P * P + 2 * P; }

VISSM_HD inline bool adapt(float* L, const float* xi, double alpha, double eta, double target, int P, double* work) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double *A = work, *v = work + P * P, *x = v + P;
  const double d = eta * (alpha - target);
  double n2 = 0.0;
#pragma unroll
  for (int j = 0; j < P; ++j) {  // (unrolled: xi sits in registers)
    x[j] = static_cast<double>(xi[j]);
    const double xx = unfused(x[j] * x[j]);
    n2 = n2 + xx;
  }
  if (!(n2 > 0.0) || d == 0.0 || !(::fabs(d) <= 1.7976931348623157e308)) return false;
  const double s = ::sqrt(::fabs(d) / n2), sgn = d > 0.0 ? 1.0 : -1.0;
#pragma unroll 1
  for (int p = 0; p < P; ++p) {
    double w = 0.0;
#pragma unroll 1
    for (int j = 0; j <= p; ++j) {
      const double a = static_cast<double>(L[p * P + j]);
      A[p * P + j] = a;
      const double t = unfused(a * x[j]);
      w = w + t;
    }
    v[p] = w * s;
  }
#pragma unroll 1
  for (int k = 0; k < P; ++k) {
    const double akk = A[k * P + k], vk = v[k];
    const double vv = vk * vk, sv = unfused(sgn * vv);
    const double r2 = unfused(akk * akk) + sv;
    if (!(akk > 0.0) || !(r2 > 0.0)) return false;
    const double rho = ::sqrt(r2), c = rho / akk, t = vk / akk;
    A[k * P + k] = rho;
#pragma unroll 1
    for (int i = k + 1; i < P; ++i) {
      const double vi = v[i];
      const double tv = t * vi, stv = unfused(sgn * tv);
      const double aik = (A[i * P + k] + stv) / c;
      A[i * P + k] = aik;
      const double cv = unfused(c * vi), tl = unfused(t * aik);
      v[i] = cv - tl;
    }
  }
#pragma unroll 1
  for (int p = 0; p < P; ++p) {
#pragma unroll 1
    for (int j = 0; j <= p; ++j) {
      const float f = static_cast<float>(A[p * P + j]);
      if (!(::fabsf(f) <= 3.4028234e38f) || (j == p && !(f > 0.f))) return false;
    }
  }
#pragma unroll 1
  for (int p = 0; p < P; ++p) {
#pragma unroll 1
    for (int j = 0; j <= p; ++j) L[p * P + j] = static_cast<float>(A[p * P + j]);
  }
  return true;
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
