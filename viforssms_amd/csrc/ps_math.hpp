// Shared math of the particle smoother (smooth.hip; include/vissm.h vissm_particle_smooth): backward simulation over
// the cloud the bootstrap filter wrote.  The cloud's particles are equally weighted (post-resampling), so the backward
// weight of particle i for a trajectory whose next state is xt is the transition density p(xt | x_i, theta) alone.
// __host__ __device__, so the CPU test-suite checks the very code the kernel runs (hostcheck.cpp).
//
//   per theta     par  = prepare(theta, dt)          AR 1 / sd; FHN 1 / sd_1, 1 / sd_2; LV e^theta and dt
//   per particle  prep = particle(x_i, par)          the transition mean; LV also the three entries of
//                                                    (dt Sigma(x_i))^-1 and -1/2 log det (it varies with i)
//   per pair      pair_logw(prep, par, xt)           the value ar_trans / lv_trans / fhn_trans return as .lp, less a
//                                                    constant of theta alone (dropped_const) that cancels
// The products are written with explicit fused multiply-adds, so every evaluation of one pair -- the maximum pass, the
// summing pass, the search, the host build -- gives the same bits.
//
// A dead particle (!sim::alive: not finite, for LV outside the positive orthant) has a NaN prep, so its logw is NaN for
// every target; the maximum passes over NaN (max_live) and pf::quantise maps NaN to 0.  A NaN target makes every logw
// NaN in the same way.
//
// Selection in integers: m = max over live i of logw_i, q_i = pf::quantise(logw_i, m), W = sum q_i (exact, at most
// 2^50 for N <= 1024), C the inclusive cumulative sum in particle order, and with U a full 32-bit word
//   tau = (U W) >> 32  (from the 128-bit product; tau < W),   idx = #{i : C_i <= tau}  <=  N - 1.
// U = .x of philox4x32_10(ctr = (t_abs, 2, lo32(r), hi32(r)), key = seed), r the trajectory's row.  The normals'
// counters carry 0 in their second word and the filter's resampling 1, so the three streams never meet.
//
// Terminal rule: at the last step of a call without x_next logw_i = 0 for every live particle (a uniform draw over the
// live ones).  W = 0 -- no live particle, or a NaN target -- gives the canonical quiet NaN at that step and idx = -1;
// a NaN target gives W = 0 at the step before it, so NaN propagates backward: a filter that died at any step (its
// cloud is NaN from there on) has all-NaN trajectories.
#pragma once
#include <stdint.h>

#include "pf_math.hpp"

namespace vissm {
namespace ps {

constexpr int kMinM = 64;

// M: a power of two, 64 <= M <= N
VHD bool valid_m(int m, int n) { return m >= kMinM && m <= n && (m & (m - 1)) == 0; }

VHD float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// floats of the per-particle part
VHD constexpr int prep_len(int model) { return model == VISSM_MODEL_LV ? 6 : model == VISSM_MODEL_FHN ? 2 : 1; }

struct Par {
  float c[6];
};
struct Prep {
  float c[6];
};

template <int MODEL>
VHD Par prepare(const float* th, float dt) {
  Par p;
  for (int i = 0; i < 6; ++i) p.c[i] = 0.f;
  if constexpr (MODEL == VISSM_MODEL_AR) {
    p.c[0] = th[0];
    p.c[1] = th[1];
    p.c[2] = 1.f / VEXP(th[2]);
  } else if constexpr (MODEL == VISSM_MODEL_LV) {
    p.c[0] = VEXP(th[0]);
    p.c[1] = VEXP(th[1]);
    p.c[2] = VEXP(th[2]);
    p.c[3] = dt;
  } else {
    const float sq = VSQRT(dt);
    p.c[0] = VEXP(th[0]);
    p.c[1] = th[1];
    p.c[2] = th[2];
    p.c[3] = dt;
    p.c[4] = 1.f / (sq * VSQRT(VEXP(th[3])));
    p.c[5] = 1.f / (sq * VSQRT(VEXP(th[4])));
  }
  return p;
}

// what pair_logw leaves out of *_trans' lp: a constant of theta (and dt) alone
template <int MODEL>
VHD float dropped_const(const float* th, float dt) {
  if constexpr (MODEL == VISSM_MODEL_AR) {
    return -th[2] - em::kHalfLog2Pi;
  } else if constexpr (MODEL == VISSM_MODEL_LV) {
    return -em::kLog2Pi_;
  } else {
    const float sq = VSQRT(dt);
    return -VLOG(sq * VSQRT(VEXP(th[3]))) - VLOG(sq * VSQRT(VEXP(th[4]))) - 2.f * em::kHalfLog2Pi;
  }
}

// the per-particle part of particle x; NaN throughout for a dead one
template <int MODEL>
VHD Prep particle(const float* x, const Par& p) {
  Prep r;
  for (int i = 0; i < 6; ++i) r.c[i] = 0.f;
  if (!sim::alive(MODEL, x)) {
    for (int i = 0; i < 6; ++i) r.c[i] = sim::quiet_nan();
    return r;
  }
  if constexpr (MODEL == VISSM_MODEL_AR) {
    r.c[0] = fma_(p.c[1], x[0], p.c[0]);
  } else if constexpr (MODEL == VISSM_MODEL_LV) {  // lv_trans's names
    const float e0 = p.c[0], e1 = p.c[1], e2 = p.c[2], dt = p.c[3];
    const float x1 = x[0], x2 = x[1];
    const float Bv = e1 * (x1 * x2);
    const float A = e0 * x1 + Bv;
    const float Cc = Bv + e2 * x2;
    const float Dl = A * Cc - Bv * Bv;
    const float inv = 1.f / (dt * Dl);
    r.c[0] = x1 + dt * (e0 * x1 - Bv);
    r.c[1] = x2 + dt * (Bv - e2 * x2);
    r.c[2] = inv * Cc;
    r.c[3] = inv * Bv;
    r.c[4] = inv * A;
    r.c[5] = -0.5f * VLOG(dt * dt * Dl);
  } else {
    const float x1 = x[0], x2 = x[1];
    const float f = x1 - x1 * x1 * x1 - x2 + p.c[1];
    r.c[0] = x1 + p.c[3] * p.c[0] * f;
    r.c[1] = x2 + p.c[3] * (p.c[2] * x1 - x2 + 1.4f);
  }
  return r;
}

// fp32 log transition density of the target xt from the particle whose per-particle part is r, less dropped_const
template <int MODEL>
VHD float pair_logw(const Prep& r, const Par& p, const float* xt) {
  // (the last operation of each branch is an explicit fma: a plain product would be contracted into the caller's
  // logw - m, and the maximum's own weight would no longer be exp(0))
  if constexpr (MODEL == VISSM_MODEL_AR) {
    const float z = (xt[0] - r.c[0]) * p.c[2];
    return fma_(-0.5f * z, z, 0.f);
  } else if constexpr (MODEL == VISSM_MODEL_LV) {
    const float q1 = xt[0] - r.c[0], q2 = xt[1] - r.c[1];
    const float g1 = fma_(r.c[2], q1, r.c[3] * q2), g2 = fma_(r.c[3], q1, r.c[4] * q2);
    const float quad = fma_(q1, g1, q2 * g2);
    return fma_(-0.5f, quad, r.c[5]);
  } else {
    const float z1 = (xt[0] - r.c[0]) * p.c[4], z2 = (xt[1] - r.c[1]) * p.c[5];
    return fma_(-0.5f * z1, z1, (-0.5f * z2) * z2);
  }
}

// the terminal rule's logw of a particle from the first float of its prep: 0 alive, NaN dead
VHD float terminal_logw(float prep0) { return prep0 == prep0 ? 0.f : sim::quiet_nan(); }

// running maximum over the live particles: NaN (a dead particle, a NaN target) is passed over
VHD float max_live(float m, float lw) { return lw > m ? lw : m; }

// tau = (U W) >> 32: U < 2^32, W <= 2^50, so the product stays below 2^82 and tau below W
VHD uint64_t threshold(uint32_t U, uint64_t W) {
  uint64_t hi, lo;
  pf::mul64(static_cast<uint64_t>(U), W, &hi, &lo);
  return (hi << 32) | (lo >> 32);
}

// the selection word of the trajectory whose Philox row is r, at absolute step t
VHD uint32_t select_u(uint64_t seed, uint32_t t, uint64_t r) {
  const u4 c{t, 2u, static_cast<uint32_t>(r), static_cast<uint32_t>(r >> 32)};
  return philox4x32_10(c, static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32)).x;
}

// serial selection (host checks): idx = #{i : C_i <= tau} from the weights q, -1 if W = 0; *W_out, *tau_out written
inline int select(const uint64_t* q, int n, uint32_t U, uint64_t* W_out, uint64_t* tau_out) {
  uint64_t W = 0;
  for (int i = 0; i < n; ++i) W += q[i];
  *W_out = W;
  *tau_out = 0;
  if (W == 0) return -1;
  const uint64_t tau = threshold(U, W);
  *tau_out = tau;
  uint64_t C = 0;
  int idx = 0;
  for (int i = 0; i < n; ++i) {
    C += q[i];
    idx += C <= tau ? 1 : 0;
  }
  return idx;
}

// one backward draw run serially (host checks): the particles x [n][S] of one step, the target xt (nullptr: the
// terminal rule), the weights into q [n]; returns idx (-1: W = 0)
template <int MODEL>
inline int draw(const float* x, int n, const float* th, float dt, const float* xt, uint32_t U, uint64_t* q,
                float* m_out) {
  constexpr int S = VISSM_MODEL_S(MODEL);
  const Par p = prepare<MODEL>(th, dt);
  float m = -__builtin_inff();
  for (int pass = 0; pass < 2; ++pass)
    for (int i = 0; i < n; ++i) {
      const Prep r = particle<MODEL>(x + static_cast<long>(i) * S, p);
      const float lw = xt ? pair_logw<MODEL>(r, p, xt) : terminal_logw(r.c[0]);
      if (pass == 0) m = max_live(m, lw);
      else q[i] = pf::quantise(lw, m, true);
    }
  *m_out = m;
  uint64_t W, tau;
  return select(q, n, U, &W, &tau);
}

}  // namespace ps
}  // namespace vissm
