// Shared math of the stochastic-volatility particle filter and smoother (sv_filter.hip; include/vissm.h
// vissm_sv_filter, vissm_sv_smooth).  SV has no obs_std / obs_bin observation model: the observed series y is the first
// coordinate of the Euler-Maruyama state and the latent log-volatility h the second (sim_math.hpp, elbo_math.hpp), with
// independent noises:
//   y_t | y_t-1, h_t-1  ~  N(y_t-1 (1 + dt th0),  dt y_t-1^2 e^{h_t-1})
//   h_t | h_t-1         ~  N(h_t-1 + dt (th1 - e^th2 h_t-1),  dt e^{2 th3})
// The weight of step t depends on the particle's state *before* the move and the move does not depend on y_t, so
// "weight on the pre-step state, resample, move" is the exactly fully adapted filter, the prior transition its
// conditional.  __host__ __device__, so the CPU test-suite checks the very code the kernels run (hostcheck.cpp).
//
//   per theta     par  = sim::prepare<SV>(theta, dt)     the constants of sim::em_step<SV>
//   per step      ob   = obs_prep(y_prev, y_now, par)    what the weight needs of the two observations: block-uniform
//   per particle  state_logw(h, ob)                      log N(y_now; y_prev (1 + dt th0), dt y_prev^2 e^h)
//                 move(h, par, n)                        coordinate 2 of sim::em_step<SV>, bit for bit, + the death rule
// Smoother (backward simulation over the filter's cloud): y_t+1 depends on h_t, so the backward weight of particle i
// for a trajectory whose next state is xt is the transition density times the particle's own weight for the *next*
// observation,  logw_i = log f(xt | h_i) + state_logw(h_i, y_next, y_next2):
//   per particle  prep = particle(h_i, ob_next, sp)      two floats: the transition mean, and state_logw
//   per pair      pair_logw(prep, sp, xt)                -1/2 ((xt - mean_i) / sd)^2 + off_i: one fma chain, one exp
// less dropped_const, a function of theta and dt alone.  The products are explicit fused multiply-adds, so every
// evaluation of one pair -- the maximum pass, the summing pass, the search, the host build -- gives the same bits.
// A dead particle (h not finite) has weight -inf in the filter and a NaN prep in the smoother (ps_math.hpp's rule).
#pragma once
#include <stdint.h>

#include "pf_math.hpp"
#include "ps_math.hpp"

namespace vissm {
namespace svf {

using ps::fma_;

// what state_logw needs of one pair of observations: logw = a e^{-h} - h / 2 + c
struct Obs {
  float a;  // -1/2 r^2 / (dt y_prev^2),  r = y_now - y_prev - dt th0 y_prev
  float c;  // -1/2 log 2 pi - log(sqrt(dt) |y_prev|)
};

VHD Obs obs_prep(float y_prev, float y_now, const sim::Par& p) {
  Obs o;
  const float r = y_now - y_prev - p.c[0] * y_prev;
  const float s = p.c[4] * (y_prev < 0.f ? -y_prev : y_prev);
  const float z = r / s;
  o.a = -0.5f * z * z;
  o.c = -em::kHalfLog2Pi - VLOG(s);
  return o;
}

// log p(y_now | y_prev, h) of the pre-step state h; -inf for a dead particle
VHD float state_logw(float h, const Obs& o) {
  if (!__builtin_isfinite(h)) return -__builtin_inff();
  return fma_(o.a, VEXP(-h), fma_(-0.5f, h, o.c));
}

VHD float state_logw(float h, float y_prev, float y_now, const sim::Par& p) {
  return state_logw(h, obs_prep(y_prev, y_now, p));
}

// the next log-volatility from h and one standard normal: the second coordinate of sim::em_step<SV> (its first, which
// needs no value here, is computed on a zero and dropped); a state that is not finite becomes the canonical quiet NaN
VHD float move(float h, const sim::Par& p, float n) {
  float x[2] = {0.f, h};
  const float nn[2] = {0.f, n};
  sim::em_step<VISSM_MODEL_SV>(x, p, nn);
  return __builtin_isfinite(x[1]) ? x[1] : sim::quiet_nan();
}

// ---- smoother -----------------------------------------------------------------------------------------------------
struct SPar {
  sim::Par p;
  float inv_sd;  // 1 / (sqrt(dt) e^th3)
};

VHD SPar sprepare(const float* th, float dt) {
  SPar s;
  s.p = sim::prepare<VISSM_MODEL_SV>(th, dt);
  s.inv_sd = 1.f / s.p.c[5];
  return s;
}

// what pair_logw leaves out of log f(xt | h_i) + state_logw: the transition's normalising constant
VHD float dropped_const(const float* th, float dt) { return -VLOG(VSQRT(dt) * VEXP(th[3])) - em::kHalfLog2Pi; }

struct Prep {
  float mean;  // h_i + dt (th1 - e^th2 h_i)
  float off;   // state_logw(h_i, next observation)
};

VHD Prep particle(float h, const Obs& next, const SPar& s) {
  Prep r;
  if (!__builtin_isfinite(h)) {
    r.mean = r.off = sim::quiet_nan();
    return r;
  }
  r.mean = fma_(s.p.c[3], fma_(-s.p.c[2], h, s.p.c[1]), h);
  r.off = state_logw(h, next);
  return r;
}

// (the last operation is an explicit fma: ps::pair_logw's note)
VHD float pair_logw(const Prep& r, const SPar& s, float xt) {
  const float z = (xt - r.mean) * s.inv_sd;
  return fma_(-0.5f * z, z, r.off);
}

// one filter step run serially (host checks): weights q [n] of the pre-step states h [n], serial systematic
// resampling with U into anc [n] (C [n] scratch), then h_out[j] moved from ancestor anc[j]'s state with normals[j].
// Returns W (0: the filter is dead, h_out all NaN); *m_out the maximum log-weight.
inline uint64_t filter_step(const float* h, int n, const float* th, float dt, float y_prev, float y_now,
                            const float* normals, uint32_t U, float* h_out, uint64_t* q, int32_t* anc, uint64_t* C,
                            float* m_out) {
  const sim::Par p = sim::prepare<VISSM_MODEL_SV>(th, dt);
  const Obs ob = obs_prep(y_prev, y_now, p);
  float m = -__builtin_inff();
  for (int pass = 0; pass < 2; ++pass)
    for (int i = 0; i < n; ++i) {
      const bool ok = __builtin_isfinite(h[i]);
      const float lw = state_logw(h[i], ob);
      if (pass == 0) m = lw > m ? lw : m;
      else q[i] = pf::quantise(lw, m, ok);
    }
  *m_out = m;
  const uint64_t W = pf::resample(q, n, U, anc, C);
  for (int j = 0; j < n; ++j) h_out[j] = W ? move(h[anc[j]], p, normals[j]) : sim::quiet_nan();
  return W;
}

// one backward draw run serially (host checks): the particles h [n] of one column, the target xt and the two
// observations after the column's (have_next = 0: the terminal rule, xt and the observations unused); the weights into
// q [n]; returns idx (-1: W = 0)
inline int draw(const float* h, int n, const float* th, float dt, int have_next, float xt, float y_next, float y_next2,
                uint32_t U, uint64_t* q, float* m_out) {
  const SPar s = sprepare(th, dt);
  Obs ob;
  ob.a = ob.c = 0.f;
  if (have_next) ob = obs_prep(y_next, y_next2, s.p);
  float m = -__builtin_inff();
  for (int pass = 0; pass < 2; ++pass)
    for (int i = 0; i < n; ++i) {
      const Prep r = particle(h[i], ob, s);
      const float lw = have_next ? pair_logw(r, s, xt) : ps::terminal_logw(r.mean);
      if (pass == 0) m = ps::max_live(m, lw);
      else q[i] = pf::quantise(lw, m, true);
    }
  *m_out = m;
  uint64_t W, tau;
  return ps::select(q, n, U, &W, &tau);
}

}  // namespace svf
}  // namespace vissm
