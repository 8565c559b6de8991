// Shared math of the fully adapted particle filter (particle.hip; include/vissm.h vissm_particle_filter_adapted) for
// AR, LV and FHN.  The Euler-Maruyama transition of sim_math.hpp is Gaussian given the previous state x,
//   x' | x ~ N(mu(x), Sigma(x)),
// and the observation reads a subset O of the coordinates with N(0, R) noise, R = obs_std^2, so the predictive
// p(y | x) and the conditional p(x' | x, y) are Gaussian in closed form.  The filter weights a particle on the former
// *before* it moves and, after the resampling, moves it by a draw from the latter.  __host__ __device__, so the CPU
// test-suite checks the very code the kernel runs (hostcheck.cpp) against numpy.linalg on the general formulas.
//
//   moments(x, par)      mu, Sigma and det Sigma from sim::prepare's Par, in em_step's parameterisation:
//                        AR  Sigma = e^{2 th2};  FHN  Sigma = diag(c[4]^2, c[5]^2);
//                        LV  Sigma = dt [[A, -Bv], [-Bv, Cc]],  det = dt^2 (e0 x1 Bv + e0 x1 e2 x2 + Bv e2 x2)
//                        (the expanded A Cc - Bv^2: three positive terms, nothing cancels)
//   logw(mo, y, bin, R)  log N(y_O; mu_O, Sigma_OO + R I) in fp32.  |O| = 1: f = Sigma_dd + R.  |O| = 2: the 2 x 2
//                        determinant det Sigma + R (Sigma_00 + Sigma_11) + R^2 and the inverse written out.
//   cond(mo, y, bin, R)  m = mu + K (y_O - mu_O), K = Sigma_.O (Sigma_OO + R I)^-1, and the lower Cholesky factor, in
//                        coordinate order, of P = Sigma - K Sigma_O. in the forms that do not cancel:
//                        one coordinate d observed (e the other):  P_dd = Sigma_dd (R / f), P_01 = Sigma_01 (R / f),
//                                                                  P_ee = Sigma_ee - Sigma_01^2 / f;
//                        both observed:  P = R K, K = [[det Sigma + R Sigma_00, R Sigma_01],
//                                                      [R Sigma_01, det Sigma + R Sigma_11]] / det(Sigma + R I);
//                        l00 = sqrt(P00), l10 = P01 / l00, l11 = sqrt(max(P11 - l10^2, 0)): the clamp keeps a radicand
//                        that rounds negative from killing the particle.
//   step(x, ...)         x'_0 = m_0 + l00 n_0,  x'_1 = m_1 + l10 n_0 + l11 n_1: em_step's convention (its L is the
//                        Cholesky factor of Sigma in the same order), so as R -> infinity the step tends to em_step.
//
// A coordinate is observed iff bin_d != 0; its value is otherwise unused.  (The bootstrap weight multiplies the
// coordinate's log-density by bin_d; every model's obs_bin is 0 / 1, where the two agree.)  y_d of an unobserved
// coordinate is not read into any result (it may be any filler, NaN included).  At least one coordinate is observed.
//
// The last operation of logw is an explicit fma (as in ps::pair_logw): a plain product would be contracted into the
// caller's logw - m, and the maximum's own weight would no longer be exp(0).  Every evaluation gives the same bits.
//
// A dead particle (NaN state) has NaN moments, logw and step; the caller gives it q = 0 (sim::alive).
#pragma once
#include "sim_math.hpp"

namespace vissm {
namespace gp {

VHD float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// transition mean, covariance (s01 = Sigma_01) and its determinant
struct Moments {
  float mu[2];
  float s00, s01, s11, det;
};

// conditional mean and lower Cholesky factor
struct Cond {
  float m[2];
  float l00, l10, l11;
};

template <int MODEL>
VHD Moments moments(const float* x, const sim::Par& p) {
  Moments r;
  r.mu[1] = 0.f;
  r.s01 = r.s11 = r.det = 0.f;
  if constexpr (MODEL == VISSM_MODEL_AR) {
    r.mu[0] = p.c[1] * x[0] + p.c[0];
    r.s00 = p.c[2] * p.c[2];
  } else if constexpr (MODEL == VISSM_MODEL_LV) {  // em_step's names
    const float e0 = p.c[0], e1 = p.c[1], e2 = p.c[2], dt = p.c[3];
    const float x1 = x[0], x2 = x[1];
    const float Bv = e1 * (x1 * x2);
    const float g1 = e0 * x1, g2 = e2 * x2;
    r.mu[0] = x1 + dt * (g1 - Bv);
    r.mu[1] = x2 + dt * (Bv - g2);
    r.s00 = dt * (g1 + Bv);
    r.s01 = -(dt * Bv);
    r.s11 = dt * (Bv + g2);
    r.det = (dt * dt) * (g1 * Bv + g1 * g2 + Bv * g2);
  } else {
    const float x1 = x[0], x2 = x[1];
    const float f = x1 - x1 * x1 * x1 - x2 + p.c[1];
    r.mu[0] = x1 + p.c[3] * p.c[0] * f;
    r.mu[1] = x2 + p.c[3] * (p.c[2] * x1 - x2 + 1.4f);
    r.s00 = p.c[4] * p.c[4];
    r.s11 = p.c[5] * p.c[5];
    r.det = r.s00 * r.s11;
  }
  return r;
}

// log N(y_O; mu_O, Sigma_OO + R I)
template <int S>
VHD float logw(const Moments& mo, const float* y, const float* bin, float R) {
  if constexpr (S == 2) {
    if (bin[0] != 0.f && bin[1] != 0.f) {
      const float a = mo.s00 + R, c = mo.s11 + R;
      const float det = mo.det + R * (mo.s00 + mo.s11) + R * R;
      const float r0 = y[0] - mo.mu[0], r1 = y[1] - mo.mu[1];
      const float quad = (c * r0 * r0 - 2.f * mo.s01 * r0 * r1 + a * r1 * r1) / det;
      return fma_(-0.5f, quad, -0.5f * VLOG(det) - em::kLog2Pi_);
    }
  }
  const bool first = S == 1 || bin[0] != 0.f;
  const float f = (first ? mo.s00 : mo.s11) + R;
  const float r = first ? y[0] - mo.mu[0] : y[S - 1] - mo.mu[S - 1];
  return fma_(-0.5f, r * r / f, -0.5f * VLOG(f) - em::kHalfLog2Pi);
}

// sqrt(max(P11 - l10^2, 0)); a NaN radicand (a dead particle) stays NaN
VHD float chol_l11(float p11, float l10) {
  const float d = p11 - l10 * l10;
  return VSQRT(d < 0.f ? 0.f : d);
}

template <int S>
VHD Cond cond(const Moments& mo, const float* y, const float* bin, float R) {
  Cond c;
  c.m[1] = 0.f;
  c.l10 = c.l11 = 0.f;
  float p00, p01 = 0.f, p11 = 0.f;
  if constexpr (S == 1) {
    const float f = mo.s00 + R;
    c.m[0] = mo.mu[0] + mo.s00 / f * (y[0] - mo.mu[0]);
    p00 = mo.s00 * (R / f);
  } else {
    if (bin[0] != 0.f && bin[1] != 0.f) {
      const float det = mo.det + R * (mo.s00 + mo.s11) + R * R;
      const float k00 = (mo.det + R * mo.s00) / det, k01 = R * mo.s01 / det, k11 = (mo.det + R * mo.s11) / det;
      const float r0 = y[0] - mo.mu[0], r1 = y[1] - mo.mu[1];
      c.m[0] = mo.mu[0] + (k00 * r0 + k01 * r1);
      c.m[1] = mo.mu[1] + (k01 * r0 + k11 * r1);
      p00 = R * k00;
      p01 = R * k01;
      p11 = R * k11;
    } else if (bin[0] != 0.f) {
      const float f = mo.s00 + R, r = y[0] - mo.mu[0], g = R / f;
      c.m[0] = mo.mu[0] + mo.s00 / f * r;
      c.m[1] = mo.mu[1] + mo.s01 / f * r;
      p00 = mo.s00 * g;
      p01 = mo.s01 * g;
      p11 = mo.s11 - mo.s01 * mo.s01 / f;
    } else {
      const float f = mo.s11 + R, r = y[1] - mo.mu[1], g = R / f;
      c.m[0] = mo.mu[0] + mo.s01 / f * r;
      c.m[1] = mo.mu[1] + mo.s11 / f * r;
      p00 = mo.s00 - mo.s01 * mo.s01 / f;
      p01 = mo.s01 * g;
      p11 = mo.s11 * g;
    }
  }
  c.l00 = VSQRT(p00);
  if constexpr (S == 2) {
    c.l10 = p01 / c.l00;
    c.l11 = chol_l11(p11, c.l10);
  }
  return c;
}

// x <- a draw from p(x' | x, y) with the standard normals n[0 .. S), without the death rule
template <int MODEL>
VHD void step(float* x, const sim::Par& p, const float* y, const float* bin, float R, const float* n) {
  constexpr int S = VISSM_MODEL_S(MODEL);
  const Cond c = cond<S>(moments<MODEL>(x, p), y, bin, R);
  x[0] = c.m[0] + c.l00 * n[0];
  if constexpr (S == 2) x[1] = c.m[1] + (c.l10 * n[0] + c.l11 * n[1]);
}

// the step with sim::advance's death rule
template <int MODEL>
VHD void advance(float* x, const sim::Par& p, const float* y, const float* bin, float R, const float* n) {
  constexpr int S = VISSM_MODEL_S(MODEL);
  step<MODEL>(x, p, y, bin, R, n);
  const bool ok = sim::alive(MODEL, x);
  for (int d = 0; d < S; ++d)
    if (!ok) x[d] = sim::quiet_nan();
}

// the predictive log-weight of the pre-step state x
template <int MODEL>
VHD float state_logw(const float* x, const sim::Par& p, const float* y, const float* bin, float R) {
  return logw<VISSM_MODEL_S(MODEL)>(moments<MODEL>(x, p), y, bin, R);
}

}  // namespace gp
}  // namespace vissm
