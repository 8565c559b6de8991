// One Euler-Maruyama step of each of the four SDE models, in the parameterisation whose transition density
// elbo_math.hpp scores (theta raw: logs where *_trans exponentiates them), so a path simulated here has the density
// that *_trans evaluates.  Shared by the forecast kernel (simulate.hip) and a host build (hostcheck.cpp) that the CPU
// test-suite checks against a float64 restatement.
//
//   AR  : x' = th1 x + th0 + e^th2 n0
//   LV  : x' = x + dt (e0 x1 - Bv, Bv - e2 x2) + sqrt(dt) L n,  L L^T = [[A, -Bv], [-Bv, Cc]]  (lv_trans's names)
//   SV  : x1' = x1 + dt th0 x1 + sqrt(dt) x1 e^{x2/2} n0;  x2' = x2 + dt (th1 - e^th2 x2) + sqrt(dt) e^th3 n1
//   FHN : x' = x + dt (e^th0 (x1 - x1^3 - x2 + th1), th2 x1 - x2 + 1.4) + sqrt(dt) (sqrt(e^th3) n0, sqrt(e^th4) n1)
//
// A sample whose new state fails alive() is dead: its state becomes the canonical quiet NaN, which every step
// propagates, so the dead step and all later ones are NaN.
#pragma once
#include "../../include/vissm.h"
#include "elbo_math.hpp"

namespace vissm {
namespace sim {

constexpr int kMaxS = 2;  // state coordinates: VISSM_MODEL_S
constexpr int kMaxP = 5;  // theta length: VISSM_MODEL_P

VHD float quiet_nan() { return __builtin_nanf(""); }

// a state the simulation may continue from: finite, and for LV inside the positive orthant
VHD bool alive(int model, const float* x) {
  const int S = VISSM_MODEL_S(model);
  bool ok = true;
  for (int d = 0; d < S; ++d) {
    ok = ok && __builtin_isfinite(x[d]);
    if (model == VISSM_MODEL_LV) ok = ok && x[d] > 0.f;
  }
  return ok;
}

// what depends on theta and dt only: computed once per sample, outside the time loop
struct Par {
  float c[6];
};

template <int MODEL>
VHD Par prepare(const float* th, float dt) {
  Par p;
  for (int i = 0; i < 6; ++i) p.c[i] = 0.f;
  if constexpr (MODEL == VISSM_MODEL_AR) {
    p.c[0] = th[0];
    p.c[1] = th[1];
    p.c[2] = VEXP(th[2]);
  } else if constexpr (MODEL == VISSM_MODEL_LV) {
    p.c[0] = VEXP(th[0]);
    p.c[1] = VEXP(th[1]);
    p.c[2] = VEXP(th[2]);
    p.c[3] = dt;
    p.c[4] = VSQRT(dt);
  } else if constexpr (MODEL == VISSM_MODEL_SV) {
    p.c[0] = dt * th[0];
    p.c[1] = th[1];
    p.c[2] = VEXP(th[2]);
    p.c[3] = dt;
    p.c[4] = VSQRT(dt);
    p.c[5] = VSQRT(dt) * VEXP(th[3]);
  } else {
    p.c[0] = VEXP(th[0]);
    p.c[1] = th[1];
    p.c[2] = th[2];
    p.c[3] = dt;
    p.c[4] = VSQRT(dt) * VSQRT(VEXP(th[3]));
    p.c[5] = VSQRT(dt) * VSQRT(VEXP(th[4]));
  }
  return p;
}

// x <- the next state from standard normals n[0 .. S)
template <int MODEL>
VHD void em_step(float* x, const Par& p, const float* n) {
  if constexpr (MODEL == VISSM_MODEL_AR) {
    x[0] = p.c[1] * x[0] + p.c[0] + p.c[2] * n[0];
  } else if constexpr (MODEL == VISSM_MODEL_LV) {
    const float e0 = p.c[0], e1 = p.c[1], e2 = p.c[2], dt = p.c[3], sq = p.c[4];
    const float x1 = x[0], x2 = x[1];
    const float Bv = e1 * (x1 * x2);
    const float A = e0 * x1 + Bv;   // a^2
    const float Cc = Bv + e2 * x2;  // b^2 + c^2
    const float m1 = dt * (e0 * x1 - Bv), m2 = dt * (Bv - e2 * x2);
    const float a = VSQRT(A);
    const float b = -Bv / a;
    const float c = VSQRT(Cc - b * b);
    x[0] = x1 + m1 + sq * a * n[0];
    x[1] = x2 + m2 + sq * (b * n[0] + c * n[1]);
  } else if constexpr (MODEL == VISSM_MODEL_SV) {
    const float x1 = x[0], x2 = x[1];
    x[0] = x1 + p.c[0] * x1 + p.c[4] * x1 * VEXP(0.5f * x2) * n[0];
    x[1] = x2 + p.c[3] * (p.c[1] - p.c[2] * x2) + p.c[5] * n[1];
  } else {
    const float x1 = x[0], x2 = x[1];
    const float f = x1 - x1 * x1 * x1 - x2 + p.c[1];
    x[0] = x1 + p.c[3] * p.c[0] * f + p.c[4] * n[0];
    x[1] = x2 + p.c[3] * (p.c[2] * x1 - x2 + 1.4f) + p.c[5] * n[1];
  }
}

// a start state that cannot be continued from is a dead row
template <int MODEL>
VHD void start(float* x) {
  if (!alive(MODEL, x))
    for (int d = 0; d < VISSM_MODEL_S(MODEL); ++d) x[d] = quiet_nan();
}

// one step with the death rule; with y != nullptr also the observation y[d] = x'[d] + obs_std n[S + d]
template <int MODEL>
VHD void advance(float* x, const Par& p, const float* n, float obs_std, float* y) {
  constexpr int S = VISSM_MODEL_S(MODEL);
  em_step<MODEL>(x, p, n);
  const bool ok = alive(MODEL, x);
  for (int d = 0; d < S; ++d) {
    if (!ok) x[d] = quiet_nan();
    if (y) y[d] = ok ? x[d] + obs_std * n[S + d] : quiet_nan();
  }
}

// run-time dispatch (host checks): one bare step without the death rule, and a whole path with it
inline void step_rt(int model, const float* x, const float* th, float dt, const float* n, float* out) {
  for (int d = 0; d < VISSM_MODEL_S(model); ++d) out[d] = x[d];
  switch (model) {
    case VISSM_MODEL_AR: em_step<VISSM_MODEL_AR>(out, prepare<VISSM_MODEL_AR>(th, dt), n); break;
    case VISSM_MODEL_LV: em_step<VISSM_MODEL_LV>(out, prepare<VISSM_MODEL_LV>(th, dt), n); break;
    case VISSM_MODEL_SV: em_step<VISSM_MODEL_SV>(out, prepare<VISSM_MODEL_SV>(th, dt), n); break;
    default: em_step<VISSM_MODEL_FHN>(out, prepare<VISSM_MODEL_FHN>(th, dt), n); break;
  }
}

// normals [H][n_stream] (n_stream = S, or 2 S with observations), x / y [S][H], x_end [S]
template <int MODEL>
inline void path(const float* x_start, const float* th, float dt, float obs_std, int H, const float* normals,
                 float* x_out, float* y_out, float* x_end) {
  constexpr int S = VISSM_MODEL_S(MODEL);
  const int NS = y_out ? 2 * S : S;
  const Par p = prepare<MODEL>(th, dt);
  float x[kMaxS] = {0.f, 0.f}, y[kMaxS] = {0.f, 0.f};
  for (int d = 0; d < S; ++d) x[d] = x_start[d];
  start<MODEL>(x);
  for (int t = 0; t < H; ++t) {
    advance<MODEL>(x, p, normals + static_cast<long>(t) * NS, obs_std, y_out ? y : nullptr);
    for (int d = 0; d < S; ++d) {
      x_out[static_cast<long>(d) * H + t] = x[d];
      if (y_out) y_out[static_cast<long>(d) * H + t] = y[d];
    }
  }
  for (int d = 0; d < S; ++d) x_end[d] = x[d];
}

inline void path_rt(int model, const float* x_start, const float* th, float dt, float obs_std, int H,
                    const float* normals, float* x_out, float* y_out, float* x_end) {
  switch (model) {
    case VISSM_MODEL_AR: path<VISSM_MODEL_AR>(x_start, th, dt, obs_std, H, normals, x_out, y_out, x_end); break;
    case VISSM_MODEL_LV: path<VISSM_MODEL_LV>(x_start, th, dt, obs_std, H, normals, x_out, y_out, x_end); break;
    case VISSM_MODEL_SV: path<VISSM_MODEL_SV>(x_start, th, dt, obs_std, H, normals, x_out, y_out, x_end); break;
    default: path<VISSM_MODEL_FHN>(x_start, th, dt, obs_std, H, normals, x_out, y_out, x_end); break;
  }
}

}  // namespace sim
}  // namespace vissm
