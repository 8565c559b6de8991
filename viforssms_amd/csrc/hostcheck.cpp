// Host (CPU) build of elbo_math.hpp so the CPU test-suite can check the
// hand-derived transition gradients against the oracle's autograd without a GPU,
// of sim_math.hpp (the forecast kernel's Euler-Maruyama steps) against a float64 restatement,
// of rng_math.hpp (Philox4x32-10 and u01) against tests/philox_ref.py,
// of pf_math.hpp (the particle filter's integer weights and resampling) against Python big-int arithmetic,
// of ps_math.hpp (the particle smoother's backward weights and integer selection) against float64 and big ints,
// of gp_math.hpp (the adapted filter's predictive weight and conditional draw) against numpy.linalg in float64,
// of svf_math.hpp (the stochastic-volatility filter's weight and move, the smoother's pair weight) against float64,
// of mh_math.hpp (the Metropolis-Hastings chain's words, proposal, log-prior and acceptance rule) against numpy,
// of cpm_math.hpp (the correlated chain's move of a carried normal, sort key and resampling integer) against numpy,
// and one whole iteration of the stochastic-volatility chain, run serially on mh_math.hpp and svf_math.hpp.
// Not part of the product path: libvissm_hostcheck.so is loaded only by tests/.
#include <cstddef>

#include "../../include/vissm.h"
#include "elbo_math.hpp"
#include "colstat_math.hpp"
#include "sim_math.hpp"
#include "rng_math.hpp"
#include "pf_math.hpp"
#include "ps_math.hpp"
#include "gp_math.hpp"
#include "svf_math.hpp"
#include "mh_math.hpp"
#include "cpm_math.hpp"

extern "C" {

// out = [lp, gh0, gh1, gt0, gt1, gth0..gth4]
void vissm_host_trans(int model, const float* xh, const float* xt, const float* th, float dt, float* out) {
  using namespace vissm::em;
  TG r;
  switch (model) {
    case 0: r = ar_trans(xh[0], xt[0], th); break;
    case 1: r = lv_trans(xh, xt, th, dt); break;
    case 2: r = sv_trans(xh, xt, th, dt); break;
    default: r = fhn_trans(xh, xt, th, dt); break;
  }
  out[0] = r.lp;
  out[1] = r.gh[0]; out[2] = r.gh[1];
  out[3] = r.gt[0]; out[4] = r.gt[1];
  for (int i = 0; i < 5; ++i) out[5 + i] = r.gth[i];
}

float vissm_host_sp_ildj(float y, float* gy) { return vissm::em::sp_ildj(y, gy); }

float vissm_host_obs(float x, float y, float bin, float sd, float* gx) { return vissm::em::obs_term(x, y, bin, sd, gx); }

// the column statistics' order key, its inverse and one narrowing step of the radix select (colstat_math.hpp: the
// code the kernels of colstat.hip run); hist is one (column, target)'s 256 bins
uint32_t vissm_host_colkey(float x) { return vissm::cs::colkey(x); }
float vissm_host_colkey_inv(uint32_t key) { return vissm::cs::colkey_inv(key); }
void vissm_host_col_narrow(const int32_t* hist, int32_t* rank_left, uint32_t* prefix, int pass) {
  vissm::cs::col_narrow(hist, rank_left, prefix, pass);
}

// One Euler-Maruyama step of sim_math.hpp (the code simulate.hip runs): out[0 .. S) = the next state from x, raw
// theta, dt and standard normals n[0 .. S), without the death rule
void hc_sim_step(int model, const float* x, const float* th, float dt, const float* n, float* out) {
  vissm::sim::step_rt(model, x, th, dt, n, out);
}

// H steps from given normals [H][n_stream] (n_stream = S, or 2 S when y_out is not null), with the death rule:
// x_out / y_out [S][H], x_end [S]
void hc_sim_path(int model, const float* x_start, const float* th, float dt, float obs_std, int H,
                 const float* normals, float* x_out, float* y_out, float* x_end) {
  vissm::sim::path_rt(model, x_start, th, dt, obs_std, H, normals, x_out, y_out, x_end);
}

int hc_sim_alive(int model, const float* x) { return vissm::sim::alive(model, x) ? 1 : 0; }

// The base noise's integer generator (rng_math.hpp: the code normal_base_kernel, normal_base_short_kernel and the
// forecast kernel run): one Philox4x32-10 block, and the map of an output word to a uniform in (0, 1]
void hc_philox(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  const vissm::u4 r = vissm::philox4x32_10(vissm::u4{ctr[0], ctr[1], ctr[2], ctr[3]}, key[0], key[1]);
  out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
}

float hc_u01(uint32_t w) { return vissm::u01(w); }

// The particle filter's integer half (pf_math.hpp: the code particle_filter_kernel runs): the quantised weight, one
// resampling threshold, the resampling integer, and systematic resampling run serially -- anc [n], C [n] the
// inclusive cumulative sum; returns W (0: anc untouched)
uint64_t hc_pf_quantise(float logw, float m, int alive) { return vissm::pf::quantise(logw, m, alive != 0); }
uint64_t hc_pf_threshold(uint32_t j, uint32_t U, uint64_t W, int log2n) { return vissm::pf::threshold(j, U, W, log2n); }
uint32_t hc_pf_resample_u(uint64_t seed, uint32_t t, uint64_t r) { return vissm::pf::resample_u(seed, t, r); }
uint64_t hc_pf_resample(const uint64_t* q, int n, uint32_t U, int32_t* anc, uint64_t* C) {
  return vissm::pf::resample(q, n, U, anc, C);
}
float hc_pf_logw(int model, const float* x, const float* y, const float* bin, float sd) {
  return vissm::pf::obs_logw(VISSM_MODEL_S(model), x, y, bin, sd);
}
double hc_pf_ll_increment(float m, uint64_t W, int n) { return vissm::pf::ll_increment(m, W, n); }

// The particle smoother's shared math (ps_math.hpp: the code particle_smooth_kernel runs).  hc_ps_pair_logw: logw of
// target xt from particle x (NaN for a dead one) and, in *dropped, the constant of theta it leaves out of *_trans' lp;
// hc_ps_select: idx = #{i : C_i <= tau} (-1: W = 0) with W and tau written; hc_ps_draw: one whole backward draw run
// serially over the particles x [n][S] (xt = NULL: the terminal rule), the weights into q [n], the maximum into *m.
float hc_ps_pair_logw(int model, const float* x, const float* xt, const float* th, float dt, float* dropped) {
  using namespace vissm::ps;
  switch (model) {
    case VISSM_MODEL_AR: {
      const Par p = prepare<VISSM_MODEL_AR>(th, dt);
      *dropped = dropped_const<VISSM_MODEL_AR>(th, dt);
      return pair_logw<VISSM_MODEL_AR>(particle<VISSM_MODEL_AR>(x, p), p, xt);
    }
    case VISSM_MODEL_LV: {
      const Par p = prepare<VISSM_MODEL_LV>(th, dt);
      *dropped = dropped_const<VISSM_MODEL_LV>(th, dt);
      return pair_logw<VISSM_MODEL_LV>(particle<VISSM_MODEL_LV>(x, p), p, xt);
    }
    default: {
      const Par p = prepare<VISSM_MODEL_FHN>(th, dt);
      *dropped = dropped_const<VISSM_MODEL_FHN>(th, dt);
      return pair_logw<VISSM_MODEL_FHN>(particle<VISSM_MODEL_FHN>(x, p), p, xt);
    }
  }
}
uint64_t hc_ps_threshold(uint32_t U, uint64_t W) { return vissm::ps::threshold(U, W); }
uint32_t hc_ps_select_u(uint64_t seed, uint32_t t, uint64_t r) { return vissm::ps::select_u(seed, t, r); }
int hc_ps_select(const uint64_t* q, int n, uint32_t U, uint64_t* W, uint64_t* tau) {
  return vissm::ps::select(q, n, U, W, tau);
}
int hc_ps_draw(int model, const float* x, int n, const float* th, float dt, const float* xt, uint32_t U, uint64_t* q,
               float* m) {
  using namespace vissm::ps;
  switch (model) {
    case VISSM_MODEL_AR: return draw<VISSM_MODEL_AR>(x, n, th, dt, xt, U, q, m);
    case VISSM_MODEL_LV: return draw<VISSM_MODEL_LV>(x, n, th, dt, xt, U, q, m);
    default: return draw<VISSM_MODEL_FHN>(x, n, th, dt, xt, U, q, m);
  }
}
int hc_ps_valid_m(int m, int n) { return vissm::ps::valid_m(m, n) ? 1 : 0; }

// The adapted filter's shared math (gp_math.hpp: the code particle_filter_kernel<.., kAdapted> runs) for the pre-step
// state x, raw theta and R = obs_std^2.  hc_gp_moments: out = [mu0, mu1, S00, S01, S11, det]; hc_gp_logw: the
// predictive log-weight; hc_gp_cond: out = [m0, m1, l00, l10, l11]; hc_gp_step: the conditional draw from normals
// n[0 .. S), without the death rule; hc_gp_l11: the clamped sqrt(P11 - l10^2).  hc_gp_filter_step: one adapted filter
// step of n particles x [n][S] run serially -- unobserved (every bin 0): sim::advance; observed: weights q [n] of the
// pre-step states, serial systematic resampling with U into anc [n] (C [n] scratch), then x_out[j] drawn from
// ancestor anc[j]'s state with normals[j], death rule applied.  Returns W (0: the filter is dead, x_out all NaN; 1 at
// an unobserved step); *m_out the maximum log-weight.
extern "C++" {
namespace {
template <int MODEL>
void gp_moments_t(const float* x, const float* th, float dt, float* out) {
  const vissm::gp::Moments mo = vissm::gp::moments<MODEL>(x, vissm::sim::prepare<MODEL>(th, dt));
  out[0] = mo.mu[0]; out[1] = mo.mu[1]; out[2] = mo.s00; out[3] = mo.s01; out[4] = mo.s11; out[5] = mo.det;
}
template <int MODEL>
void gp_cond_t(const float* x, const float* th, float dt, const float* y, const float* bin, float R, float* out) {
  using namespace vissm;
  const gp::Cond c = gp::cond<VISSM_MODEL_S(MODEL)>(gp::moments<MODEL>(x, sim::prepare<MODEL>(th, dt)), y, bin, R);
  out[0] = c.m[0]; out[1] = c.m[1]; out[2] = c.l00; out[3] = c.l10; out[4] = c.l11;
}
template <int MODEL>
uint64_t gp_filter_step_t(const float* x, int n, const float* th, float dt, const float* y, const float* bin,
                          float obs_std, const float* normals, uint32_t U, float* x_out, uint64_t* q, int32_t* anc,
                          uint64_t* C, float* m_out) {
  using namespace vissm;
  constexpr int S = VISSM_MODEL_S(MODEL);
  const sim::Par p = sim::prepare<MODEL>(th, dt);
  const float R = obs_std * obs_std;
  bool observed = false;
  for (int d = 0; d < S; ++d) observed = observed || bin[d] != 0.f;
  *m_out = 0.f;
  if (!observed) {
    for (int i = 0; i < n; ++i) {
      for (int d = 0; d < S; ++d) x_out[i * S + d] = x[i * S + d];
      sim::advance<MODEL>(x_out + i * S, p, normals + i * S, 0.f, nullptr);
      q[i] = 0;
      anc[i] = i;
    }
    return 1;
  }
  float m = -__builtin_inff();
  for (int pass = 0; pass < 2; ++pass)
    for (int i = 0; i < n; ++i) {
      const bool ok = sim::alive(MODEL, x + i * S);
      const float lw = ok ? gp::state_logw<MODEL>(x + i * S, p, y, bin, R) : -__builtin_inff();
      if (pass == 0) m = lw > m ? lw : m;
      else q[i] = pf::quantise(lw, m, ok);
    }
  *m_out = m;
  const uint64_t W = pf::resample(q, n, U, anc, C);
  for (int j = 0; j < n; ++j)
    for (int d = 0; d < S; ++d) x_out[j * S + d] = W ? x[anc[j] * S + d] : sim::quiet_nan();
  if (W)
    for (int j = 0; j < n; ++j) gp::advance<MODEL>(x_out + j * S, p, y, bin, R, normals + j * S);
  return W;
}
}  // namespace
}  // extern "C++"

void hc_gp_moments(int model, const float* x, const float* th, float dt, float* out) {
  switch (model) {
    case VISSM_MODEL_AR: gp_moments_t<VISSM_MODEL_AR>(x, th, dt, out); break;
    case VISSM_MODEL_LV: gp_moments_t<VISSM_MODEL_LV>(x, th, dt, out); break;
    default: gp_moments_t<VISSM_MODEL_FHN>(x, th, dt, out); break;
  }
}
float hc_gp_logw(int model, const float* x, const float* th, float dt, const float* y, const float* bin, float R) {
  using namespace vissm;
  switch (model) {
    case VISSM_MODEL_AR: return gp::state_logw<VISSM_MODEL_AR>(x, sim::prepare<VISSM_MODEL_AR>(th, dt), y, bin, R);
    case VISSM_MODEL_LV: return gp::state_logw<VISSM_MODEL_LV>(x, sim::prepare<VISSM_MODEL_LV>(th, dt), y, bin, R);
    default: return gp::state_logw<VISSM_MODEL_FHN>(x, sim::prepare<VISSM_MODEL_FHN>(th, dt), y, bin, R);
  }
}
void hc_gp_cond(int model, const float* x, const float* th, float dt, const float* y, const float* bin, float R,
                float* out) {
  switch (model) {
    case VISSM_MODEL_AR: gp_cond_t<VISSM_MODEL_AR>(x, th, dt, y, bin, R, out); break;
    case VISSM_MODEL_LV: gp_cond_t<VISSM_MODEL_LV>(x, th, dt, y, bin, R, out); break;
    default: gp_cond_t<VISSM_MODEL_FHN>(x, th, dt, y, bin, R, out); break;
  }
}
void hc_gp_step(int model, const float* x, const float* th, float dt, const float* y, const float* bin, float R,
                const float* n, float* out) {
  using namespace vissm;
  for (int d = 0; d < VISSM_MODEL_S(model); ++d) out[d] = x[d];
  switch (model) {
    case VISSM_MODEL_AR: gp::step<VISSM_MODEL_AR>(out, sim::prepare<VISSM_MODEL_AR>(th, dt), y, bin, R, n); break;
    case VISSM_MODEL_LV: gp::step<VISSM_MODEL_LV>(out, sim::prepare<VISSM_MODEL_LV>(th, dt), y, bin, R, n); break;
    default: gp::step<VISSM_MODEL_FHN>(out, sim::prepare<VISSM_MODEL_FHN>(th, dt), y, bin, R, n); break;
  }
}
float hc_gp_l11(float p11, float l10) { return vissm::gp::chol_l11(p11, l10); }
uint64_t hc_gp_filter_step(int model, const float* x, int n, const float* th, float dt, const float* y,
                           const float* bin, float obs_std, const float* normals, uint32_t U, float* x_out,
                           uint64_t* q, int32_t* anc, uint64_t* C, float* m_out) {
  switch (model) {
    case VISSM_MODEL_AR:
      return gp_filter_step_t<VISSM_MODEL_AR>(x, n, th, dt, y, bin, obs_std, normals, U, x_out, q, anc, C, m_out);
    case VISSM_MODEL_LV:
      return gp_filter_step_t<VISSM_MODEL_LV>(x, n, th, dt, y, bin, obs_std, normals, U, x_out, q, anc, C, m_out);
    default:
      return gp_filter_step_t<VISSM_MODEL_FHN>(x, n, th, dt, y, bin, obs_std, normals, U, x_out, q, anc, C, m_out);
  }
}

// The stochastic-volatility filter's and smoother's shared math (svf_math.hpp: the code sv_filter_kernel and
// sv_smooth_kernel run), theta raw [4].  hc_svf_logw: the weight of the pre-step state h for (y_prev, y_now);
// hc_svf_move: the next h from one normal, with the death rule; hc_svf_pair_logw: the backward weight of particle h for
// target xt with the next two observations, *dropped the constant it leaves out; hc_svf_filter_step and hc_svf_draw:
// one whole filter step and one whole backward draw run serially (svf::filter_step, svf::draw).
float hc_svf_logw(float h, float y_prev, float y_now, const float* th, float dt) {
  return vissm::svf::state_logw(h, y_prev, y_now, vissm::sim::prepare<VISSM_MODEL_SV>(th, dt));
}
float hc_svf_move(float h, const float* th, float dt, float n) {
  return vissm::svf::move(h, vissm::sim::prepare<VISSM_MODEL_SV>(th, dt), n);
}
float hc_svf_pair_logw(float h, float xt, float y_next, float y_next2, const float* th, float dt, float* dropped) {
  using namespace vissm::svf;
  const SPar s = sprepare(th, dt);
  *dropped = dropped_const(th, dt);
  return pair_logw(particle(h, obs_prep(y_next, y_next2, s.p), s), s, xt);
}
uint64_t hc_svf_filter_step(const float* h, int n, const float* th, float dt, float y_prev, float y_now,
                            const float* normals, uint32_t U, float* h_out, uint64_t* q, int32_t* anc, uint64_t* C,
                            float* m_out) {
  return vissm::svf::filter_step(h, n, th, dt, y_prev, y_now, normals, U, h_out, q, anc, C, m_out);
}
int hc_svf_draw(const float* h, int n, const float* th, float dt, int have_next, float xt, float y_next, float y_next2,
                uint32_t U, uint64_t* q, float* m) {
  return vissm::svf::draw(h, n, th, dt, have_next, xt, y_next, y_next2, U, q, m);
}

// The Metropolis-Hastings chain's shared math (mh_math.hpp: the code pmmh_kernel runs).  hc_mh_row: the first Philox
// row of iteration i of chain c; hc_mh_words: the block of group g; hc_mh_uniform / hc_mh_log_uniform: the decision's u
// and log u from a word; hc_mh_xi: the eight normals of row r from box_muller4_ref (the kernel's come from the hardware
// transcendentals); hc_mh_propose: theta' [P]; hc_mh_log_prior; hc_mh_accept: the decision.
uint64_t hc_mh_row(uint64_t row0, uint64_t i, uint64_t C, uint64_t c, uint64_t N) {
  return vissm::mh::row_of(row0, i, C, c, N);
}
void hc_mh_words(uint32_t g, uint64_t r, uint64_t seed, uint32_t out[4]) {
  const vissm::u4 w = vissm::mh::words(g, r, seed);
  out[0] = w.x; out[1] = w.y; out[2] = w.z; out[3] = w.w;
}
double hc_mh_uniform(uint32_t x) { return vissm::mh::uniform(x); }
double hc_mh_log_uniform(uint32_t x) { return vissm::mh::log_uniform(x); }
void hc_mh_xi(uint64_t r, uint64_t seed, float out[8]) {
  vissm::mh::box_muller4_ref(vissm::mh::words(0u, r, seed), out);
  vissm::mh::box_muller4_ref(vissm::mh::words(1u, r, seed), out + 4);
}
void hc_mh_propose(const float* th, const float* L, const float* xi, int P, float* out) {
  vissm::mh::propose(th, L, xi, P, out);
}
double hc_mh_log_prior(const float* th, const float* prior, int P) { return vissm::mh::log_prior(th, prior, P); }
int hc_mh_accept(double logu, double ll_prop, double ll_cur, double lp_prop, double lp_cur) {
  return vissm::mh::accept(logu, ll_prop, ll_cur, lp_prop, lp_cur) ? 1 : 0;
}

// The adaptive chain's update (mh_math.hpp: the code thread 0 of pmmh_kernel<.., ADAPT = true> runs).  hc_mh_alpha:
// the acceptance probability from the state before the decision; hc_mh_eta: the step size of the absolute iteration
// i; hc_mh_adapt: L [P][P] -> L' in place from the normals xi [P], returns 1 when L changed, 0 when it was kept.
double hc_mh_alpha(double ll_prop, double ll_cur, double lp_prop, double lp_cur) {
  return vissm::mh::accept_prob(ll_prop, ll_cur, lp_prop, lp_cur);
}
double hc_mh_eta(int P, int64_t i, double gamma) { return vissm::mh::adapt_eta(P, i, gamma); }
int hc_mh_adapt(float* L, const float* xi, double alpha, double eta, double target, int P) {
  if (P < 1 || P > vissm::mh::kMaxP) return -1;
  double work[vissm::mh::adapt_work(vissm::mh::kMaxP)];
  return vissm::mh::adapt(L, xi, alpha, eta, target, P, work) ? 1 : 0;
}

// The correlated chain's shared math (cpm_math.hpp: the code sv_filter_sorted_kernel and sv_cpmmh_kernel run).
// hc_cpm_cn: the autoregressive move of one carried normal; hc_cpm_sigma: sqrt(1 - rho^2) as the entry rounds it;
// hc_cpm_valid_rho: the entry's refusal; hc_cpm_sort_key / hc_cpm_key_value: the sort key and its inverse;
// hc_cpm_resample_u: the 24-bit resampling integer of a carried normal.
float hc_cpm_cn(float u, float eps, float rho, float sigma) { return vissm::cpm::cn(u, eps, rho, sigma); }
float hc_cpm_sigma(float rho) { return vissm::cpm::sigma_of(rho); }
int hc_cpm_valid_rho(float rho) { return vissm::cpm::valid_rho(rho) ? 1 : 0; }
uint32_t hc_cpm_sort_key(float h) { return vissm::cpm::sort_key(h); }
float hc_cpm_key_value(uint32_t k) { return vissm::cpm::key_value(k); }
uint32_t hc_cpm_resample_u(float ur) { return vissm::cpm::resample_u(ur); }

// One iteration of one stochastic-volatility chain (sv_pmmh_kernel's, pmmh.hip) run serially on mh_math.hpp and
// svf::filter_step: iteration i of chain c of C with n particles from the state theta [4] with the estimate ll_cur.
// The proposal's normals come from box_muller4_ref, the filter's from the same formula on the Philox counter
// (ta / 4, 0, lo32(row), hi32(row)), entry ta % 4, of row = r + lane; the resampling integer is pf::resample_u(seed, ta,
// r).  The filter starts every particle at h_start (not finite: the quiet NaN) over y [T + 1] and leaves at W = 0 with
// ll' = -inf.  theta_prop [4]; out = {lp, lp', log u, ll'}; optional traces: h_tr [T + 1][n] the states before each step
// and after the last, q_tr and anc_tr [T][n], n_tr [T][n] the normals, m_tr and W_tr [T] (rows past a death are left
// untouched).  Returns the decision.
int hc_svpmmh_iteration(uint64_t seed, uint64_t row0, uint64_t i, uint64_t C, uint64_t c, int n, int T, float dt,
                        const float* theta, double ll_cur, const float* L, const float* prior, float h_start,
                        const float* y, float* theta_prop, double* out, float* h_tr, uint64_t* q_tr, int32_t* anc_tr,
                        float* n_tr, float* m_tr, uint64_t* W_tr) {
  using namespace vissm;
  constexpr int P = VISSM_MODEL_P(VISSM_MODEL_SV);
  if (n < 1 || n > pf::kMaxN || T < 0) return -1;
  const uint64_t r = mh::row_of(row0, i, C, c, static_cast<uint64_t>(n));
  float xi[8];
  mh::box_muller4_ref(mh::words(0u, r, seed), xi);
  mh::box_muller4_ref(mh::words(1u, r, seed), xi + 4);
  mh::propose(theta, L, xi, P, theta_prop);
  const uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
  float h[pf::kMaxN], hn[pf::kMaxN], nn[pf::kMaxN];
  uint64_t q[pf::kMaxN], Cs[pf::kMaxN];
  int32_t anc[pf::kMaxN];
  for (int p = 0; p < n; ++p) h[p] = __builtin_isfinite(h_start) ? h_start : sim::quiet_nan();
  double llp = 0.0;
  for (int ta = 0; ta < T; ++ta) {
    for (int p = 0; p < n; ++p) {
      const uint64_t row = r + static_cast<uint64_t>(p);
      const u4 ctr{static_cast<uint32_t>(ta) >> 2, 0u, static_cast<uint32_t>(row), static_cast<uint32_t>(row >> 32)};
      float v[4];
      mh::box_muller4_ref(philox4x32_10(ctr, k0, k1), v);
      nn[p] = v[ta & 3];
    }
    float m = 0.f;
    const uint64_t W = svf::filter_step(h, n, theta_prop, dt, y[ta], y[ta + 1], nn,
                                        pf::resample_u(seed, static_cast<uint32_t>(ta), r), hn, q, anc, Cs, &m);
    const size_t o = static_cast<size_t>(ta) * n;
    for (int p = 0; p < n; ++p) {
      if (h_tr) h_tr[o + p] = h[p];
      if (q_tr) q_tr[o + p] = q[p];
      if (anc_tr) anc_tr[o + p] = W ? anc[p] : -1;
      if (n_tr) n_tr[o + p] = nn[p];
      if (h_tr) h_tr[o + n + p] = hn[p];
      h[p] = hn[p];
    }
    if (m_tr) m_tr[ta] = m;
    if (W_tr) W_tr[ta] = W;
    if (W == 0) {
      llp = -__builtin_inf();
      break;
    }
    llp += pf::ll_increment(m, W, n);
  }
  const double lp = mh::log_prior(theta, prior, P), lpp = mh::log_prior(theta_prop, prior, P);
  const double logu = mh::log_uniform(mh::words(2u, r, seed).x);
  out[0] = lp;
  out[1] = lpp;
  out[2] = logu;
  out[3] = llp;
  return mh::accept(logu, llp, ll_cur, lpp, lp) ? 1 : 0;
}

// the C ABI's struct layouts as the C compiler sees them (the ctypes mirrors in viforssms_amd/_lib.py are
// checked against these): which = 0 VissmFlowDesc, 1 VissmFlowParams, 2 VissmFlowGrads, 3 VissmElboData, 4 VissmColStatDesc, 5 VissmSimDesc, 6 VissmPfDesc, 7 VissmPsDesc, 8 VissmPmmhDesc; out = {size,
// offset of the last field}
void vissm_host_abi_layout(int which, size_t* out) {
  switch (which) {
    case 0: out[0] = sizeof(VissmFlowDesc); out[1] = offsetof(VissmFlowDesc, out_pitch); break;
    case 1: out[0] = sizeof(VissmFlowParams); out[1] = offsetof(VissmFlowParams, theta_rank); break;
    case 2: out[0] = sizeof(VissmFlowGrads); out[1] = offsetof(VissmFlowGrads, b_head); break;
    case 5: out[0] = sizeof(VissmSimDesc); out[1] = offsetof(VissmSimDesc, with_obs); break;
    case 4: out[0] = sizeof(VissmColStatDesc); out[1] = offsetof(VissmColStatDesc, n_ranks); break;
    case 6: out[0] = sizeof(VissmPfDesc); out[1] = offsetof(VissmPfDesc, obs_std); break;
    case 7: out[0] = sizeof(VissmPsDesc); out[1] = offsetof(VissmPsDesc, dt); break;
    case 8: out[0] = sizeof(VissmPmmhDesc); out[1] = offsetof(VissmPmmhDesc, obs_std); break;
    default: out[0] = sizeof(VissmElboData); out[1] = offsetof(VissmElboData, obs_stride); break;
  }
}

}
