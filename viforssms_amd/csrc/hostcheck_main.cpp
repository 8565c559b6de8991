// Sanitizer driver for the host build of elbo_math.hpp (hostcheck.cpp): built with
// -fsanitize=address,undefined into build/hostcheck_san and run by the CPU test-suite
// (tests/test_lib.py::test_hostcheck_sanitized).  Each model's hand-derived transition
// gradient is checked against central finite differences of its own log-density over
// a fixed pseudo-random grid of states and parameters, and the ABI layout query is
// exercised; the column statistics' order key, its inverse and the radix select's narrowing
// step (colstat_math.hpp) are checked against the floats' own order and std::nth_element;
// the forecast's Euler-Maruyama steps (sim_math.hpp) are run for each model against a double restatement, over a
// dying LV row and over H = 0 and 1;
// the base noise's Philox4x32-10 (rng_math.hpp) is run on the Random123 known-answer vectors and, against a
// restatement with separate high and low multiplies, on a few thousand counters; u01 on the ends of its range;
// the particle filter's quantised weights, thresholds and serial systematic resampling (pf_math.hpp) on their edge
// cases against a 128-bit restatement;
// the particle smoother's backward weights, integer selection and whole draws (ps_math.hpp) on theirs;
// the adapted filter's predictive weight, conditional mean and Cholesky factor (gp_math.hpp) against a double
// restatement of the general 2 x 2 formulas over every mask and obs_std from 0.05 to 1000 transition sd, the clamp,
// and whole serial filter steps with dead particles;
// the stochastic-volatility filter's weight and move and the smoother's pair weight (svf_math.hpp) against a double
// restatement, sim_math.hpp's own SV step and sv_trans' joint density, with whole serial steps and draws;
// the Metropolis-Hastings chain's words, uniform, proposal, log-prior and acceptance rule (mh_math.hpp) on their edge
// cases: the counter's second word, u inside (0, 1), a zero factor, the -inf and NaN decisions;
// whole iterations of the stochastic-volatility chain run serially (hc_svpmmh_iteration): a zero factor proposes theta
// itself, the traces rebuild ll', a zero in the series and a state that is not finite kill the proposal;
// the adaptive chain's factor update (mh::adapt): updates and downdates at P = 3, 4, 5 against the rank-one identity, the
// r2 <= 0 guard, an fp32-underflowing diagonal and xi = 0;
// any sanitizer report aborts the run (-fno-sanitize-recover=all).
// Exit 0 = all checks passed.  Not part of the product path.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <algorithm>
#include <initializer_list>
#include <vector>

extern "C" {
void vissm_host_trans(int model, const float* xh, const float* xt, const float* th, float dt, float* out);
float vissm_host_sp_ildj(float y, float* gy);
float vissm_host_obs(float x, float y, float bin, float sd, float* gx);
void vissm_host_abi_layout(int which, size_t* out);
uint32_t vissm_host_colkey(float x);
float vissm_host_colkey_inv(uint32_t key);
void vissm_host_col_narrow(const int32_t* hist, int32_t* rank_left, uint32_t* prefix, int pass);
void hc_sim_step(int model, const float* x, const float* th, float dt, const float* n, float* out);
void hc_sim_path(int model, const float* x_start, const float* th, float dt, float obs_std, int H,
                 const float* normals, float* x_out, float* y_out, float* x_end);
void hc_philox(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
float hc_u01(uint32_t w);
uint64_t hc_pf_quantise(float logw, float m, int alive);
uint64_t hc_pf_threshold(uint32_t j, uint32_t U, uint64_t W, int log2n);
uint32_t hc_pf_resample_u(uint64_t seed, uint32_t t, uint64_t r);
uint64_t hc_pf_resample(const uint64_t* q, int n, uint32_t U, int32_t* anc, uint64_t* C);
double hc_pf_ll_increment(float m, uint64_t W, int n);
float hc_ps_pair_logw(int model, const float* x, const float* xt, const float* th, float dt, float* dropped);
uint64_t hc_ps_threshold(uint32_t U, uint64_t W);
uint32_t hc_ps_select_u(uint64_t seed, uint32_t t, uint64_t r);
int hc_ps_select(const uint64_t* q, int n, uint32_t U, uint64_t* W, uint64_t* tau);
int hc_ps_draw(int model, const float* x, int n, const float* th, float dt, const float* xt, uint32_t U, uint64_t* q,
               float* m);
void hc_gp_moments(int model, const float* x, const float* th, float dt, float* out);
float hc_gp_logw(int model, const float* x, const float* th, float dt, const float* y, const float* bin, float R);
void hc_gp_cond(int model, const float* x, const float* th, float dt, const float* y, const float* bin, float R,
                float* out);
void hc_gp_step(int model, const float* x, const float* th, float dt, const float* y, const float* bin, float R,
                const float* n, float* out);
float hc_gp_l11(float p11, float l10);
uint64_t hc_gp_filter_step(int model, const float* x, int n, const float* th, float dt, const float* y,
                           const float* bin, float obs_std, const float* normals, uint32_t U, float* x_out,
                           uint64_t* q, int32_t* anc, uint64_t* C, float* m_out);
float hc_svf_logw(float h, float y_prev, float y_now, const float* th, float dt);
float hc_svf_move(float h, const float* th, float dt, float n);
float hc_svf_pair_logw(float h, float xt, float y_next, float y_next2, const float* th, float dt, float* dropped);
uint64_t hc_svf_filter_step(const float* h, int n, const float* th, float dt, float y_prev, float y_now,
                            const float* normals, uint32_t U, float* h_out, uint64_t* q, int32_t* anc, uint64_t* C,
                            float* m_out);
int hc_svf_draw(const float* h, int n, const float* th, float dt, int have_next, float xt, float y_next, float y_next2,
                uint32_t U, uint64_t* q, float* m);
uint64_t hc_mh_row(uint64_t row0, uint64_t i, uint64_t C, uint64_t c, uint64_t N);
void hc_mh_words(uint32_t g, uint64_t r, uint64_t seed, uint32_t out[4]);
double hc_mh_uniform(uint32_t x);
double hc_mh_log_uniform(uint32_t x);
void hc_mh_xi(uint64_t r, uint64_t seed, float out[8]);
void hc_mh_propose(const float* th, const float* L, const float* xi, int P, float* out);
double hc_mh_log_prior(const float* th, const float* prior, int P);
int hc_mh_accept(double logu, double ll_prop, double ll_cur, double lp_prop, double lp_cur);
double hc_mh_alpha(double ll_prop, double ll_cur, double lp_prop, double lp_cur);
double hc_mh_eta(int P, int64_t i, double gamma);
int hc_mh_adapt(float* L, const float* xi, double alpha, double eta, double target, int P);
float hc_cpm_cn(float u, float eps, float rho, float sigma);
float hc_cpm_sigma(float rho);
int hc_cpm_valid_rho(float rho);
uint32_t hc_cpm_sort_key(float h);
float hc_cpm_key_value(uint32_t k);
uint32_t hc_cpm_resample_u(float ur);
int hc_svpmmh_iteration(uint64_t seed, uint64_t row0, uint64_t i, uint64_t C, uint64_t c, int n, int T, float dt,
                        const float* theta, double ll_cur, const float* L, const float* prior, float h_start,
                        const float* y, float* theta_prop, double* out, float* h_tr, uint64_t* q_tr, int32_t* anc_tr,
                        float* n_tr, float* m_tr, uint64_t* W_tr);
}

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
double uniform(double lo, double hi) {  // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return lo + (hi - lo) * (static_cast<double>(z >> 11) * 0x1.0p-53);
}

float lp_of(int model, const float* xh, const float* xt, const float* th, float dt) {
  float out[10];
  vissm_host_trans(model, xh, xt, th, dt, out);
  return out[0];
}

// central difference of lp in one input coordinate (which: 0 head, 1 tail, 2 theta)
double fd(int model, float* xh, float* xt, float* th, float dt, int which, int i) {
  float* v = which == 0 ? xh : which == 1 ? xt : th;
  const float x0 = v[i];
  const float h = 1e-2f * std::fmax(1.f, std::fabs(x0));
  v[i] = x0 + h;
  const double lp_p = lp_of(model, xh, xt, th, dt);
  v[i] = x0 - h;
  const double lp_m = lp_of(model, xh, xt, th, dt);
  v[i] = x0;
  return (lp_p - lp_m) / (2.0 * (static_cast<double>(x0 + h) - static_cast<double>(x0)));
}

int check_model(int model, int cases) {
  const int D = model == 0 ? 1 : 2;
  const int P = model == 0 ? 3 : model == 1 ? 3 : model == 2 ? 4 : 5;
  const float dt = model == 0 || model == 2 ? 1.f : 0.1f;
  int bad = 0;
  for (int c = 0; c < cases; ++c) {
    float xh[2] = {0.f, 0.f}, xt[2] = {0.f, 0.f}, th[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int d = 0; d < D; ++d) {
      if (model == 1) {  // LV populations
        xh[d] = static_cast<float>(uniform(20.0, 200.0));
        xt[d] = xh[d] + static_cast<float>(uniform(-3.0, 3.0));
      } else if (model == 2 && d == 0) {  // SV: the sd s1 = sqrt(dt) x1 e^{x2/2} vanishes at x1 = 0; keep |x1| >= 0.5
        xh[d] = static_cast<float>(uniform(0.5, 2.0) * (uniform(0.0, 1.0) < 0.5 ? -1.0 : 1.0));
        xt[d] = xh[d] + static_cast<float>(uniform(-0.5, 0.5));
      } else {
        xh[d] = static_cast<float>(uniform(-2.0, 2.0));
        xt[d] = xh[d] + static_cast<float>(uniform(-0.5, 0.5));
      }
    }
    for (int p = 0; p < P; ++p) th[p] = static_cast<float>(uniform(-1.0, 1.0));
    if (model == 1) {  // LV log-rates near the reference's (log 0.5, log 0.0025, log 0.3)
      th[0] = static_cast<float>(std::log(0.5) + uniform(-0.2, 0.2));
      th[1] = static_cast<float>(std::log(0.0025) + uniform(-0.2, 0.2));
      th[2] = static_cast<float>(std::log(0.3) + uniform(-0.2, 0.2));
    }
    float out[10];
    vissm_host_trans(model, xh, xt, th, dt, out);
    if (!std::isfinite(out[0])) { std::printf("model %d case %d: lp not finite\n", model, c); ++bad; continue; }
    double gmax = 1.0;
    for (int i = 1; i < 10; ++i) gmax = std::fmax(gmax, std::fabs(out[i]));
    struct { int which, n, off; } groups[3] = {{0, D, 1}, {1, D, 3}, {2, P, 5}};
    for (const auto& g : groups)
      for (int i = 0; i < g.n; ++i) {
        const double num = fd(model, xh, xt, th, dt, g.which, i);
        const double ana = out[g.off + i];
        if (!(std::fabs(num - ana) <= 2e-2 * gmax + 2e-2 * std::fabs(num))) {
          std::printf("model %d case %d input %d.%d: analytic %.6g vs finite difference %.6g\n", model, c, g.which, i,
                      ana, num);
          ++bad;
        }
      }
  }
  return bad;
}

float from_bits(uint32_t b) {
  float x;
  std::memcpy(&x, &b, sizeof x);
  return x;
}

uint32_t to_bits(float x) {
  uint32_t b;
  std::memcpy(&b, &x, sizeof b);
  return b;
}

// key order == the floats' order with NaN last, and inverse(key(x)) == x (-0 -> +0, NaN -> NaN), over +-0,
// +-denormals, +-inf, NaNs of both signs and 10^4 random bit patterns
int check_colkey() {
  std::vector<float> v;
  for (uint32_t b : {0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x007FFFFFu, 0x807FFFFFu, 0x00800000u,
                     0x80800000u, 0x7F7FFFFFu, 0xFF7FFFFFu, 0x7F800000u, 0xFF800000u, 0x7FC00000u, 0xFFC00000u,
                     0x7F800001u, 0xFFFFFFFFu, 0x3F800000u, 0xBF800000u})
    v.push_back(from_bits(b));
  for (int i = 0; i < 10000; ++i) v.push_back(from_bits(static_cast<uint32_t>(uniform(0.0, 4294967296.0))));
  int bad = 0;
  for (size_t i = 0; i < v.size(); ++i) {
    const float x = v[i];
    const uint32_t k = vissm_host_colkey(x);
    const float back = vissm_host_colkey_inv(k);
    if (std::isnan(x)) {
      if (k != 0xFFFFFFFFu || !std::isnan(back)) { std::printf("colkey: NaN %08x -> %08x\n", to_bits(x), k); ++bad; }
      continue;
    }
    if (k == 0xFFFFFFFFu) { std::printf("colkey: %g got the NaN key\n", x); ++bad; }
    const uint32_t want = x == 0.f ? 0u : to_bits(x);
    if (to_bits(back) != want) { std::printf("colkey: %08x -> %08x -> %08x\n", to_bits(x), k, to_bits(back)); ++bad; }
  }
  for (size_t i = 0; i < v.size(); ++i)
    for (size_t j = i + 1; j < std::min(v.size(), i + 40); ++j) {
      const float a = v[i], b = v[j];
      const uint32_t ka = vissm_host_colkey(a), kb = vissm_host_colkey(b);
      const bool na = std::isnan(a), nb = std::isnan(b);
      const bool ok = na || nb ? (ka < kb) == (!na && nb) && (kb < ka) == (!nb && na)
                               : (ka < kb) == (a < b) && (kb < ka) == (b < a);
      if (!ok) { std::printf("colkey order: %g (%08x) vs %g (%08x)\n", a, ka, b, kb); ++bad; }
    }
  return bad;
}

// the 4-pass select on a host array (histogram of one key byte over the elements matching the prefix, then narrow)
// equals std::nth_element at every rank of a 300-element array with ties
int check_select() {
  std::vector<float> x(300);
  for (size_t i = 0; i < x.size(); ++i) {
    const int kind = static_cast<int>(uniform(0.0, 4.0));
    x[i] = kind == 0   ? static_cast<float>(static_cast<int>(uniform(-3.0, 4.0)))
           : kind == 1 ? static_cast<float>(uniform(-1e3, 1e3))
           : kind == 2 ? 1.f + static_cast<float>(static_cast<int>(uniform(0.0, 20.0))) * 0x1.0p-23f
                       : static_cast<float>(uniform(-1e-3, 1e-3));
  }
  x[7] = 0.f; x[8] = -0.f; x[9] = INFINITY; x[10] = -INFINITY; x[11] = from_bits(1u); x[12] = from_bits(0x80000001u);
  int bad = 0;
  for (int rank = 0; rank < static_cast<int>(x.size()); ++rank) {
    int32_t left = rank;
    uint32_t prefix = 0;
    for (int pass = 0; pass < 4; ++pass) {
      int32_t hist[256] = {0};
      const int shift = 8 * (3 - pass);
      for (float v : x) {
        const uint32_t k = vissm_host_colkey(v);
        if (pass == 0 || (k >> (shift + 8)) == (prefix >> (shift + 8))) ++hist[(k >> shift) & 255u];
      }
      vissm_host_col_narrow(hist, &left, &prefix, pass);
    }
    std::vector<float> y(x);
    std::nth_element(y.begin(), y.begin() + rank, y.end());
    const float got = vissm_host_colkey_inv(prefix);
    // +0 and -0 compare equal and either may sit at the rank: the select returns +0
    // (what is left of the rank counts the ties below it, never negative)
    if (!(got == y[rank]) || left < 0) { std::printf("select rank %d: %g vs %g (left %d)\n", rank, got, y[rank], left); ++bad; }
  }
  return bad;
}

// one step of each model in double, from the formulas of sim_math.hpp's header comment
void sim_step_ref(int model, const float* xf, const float* thf, double dt, const float* nf, double* out) {
  double x[2] = {xf[0], xf[1]}, th[5], n[2] = {nf[0], nf[1]};
  for (int i = 0; i < 5; ++i) th[i] = thf[i];
  const double sq = std::sqrt(dt);
  if (model == 0) {
    out[0] = th[1] * x[0] + th[0] + std::exp(th[2]) * n[0];
  } else if (model == 1) {
    const double e0 = std::exp(th[0]), e1 = std::exp(th[1]), e2 = std::exp(th[2]);
    const double Bv = e1 * x[0] * x[1], A = e0 * x[0] + Bv, Cc = Bv + e2 * x[1];
    const double a = std::sqrt(A), b = -Bv / a, c = std::sqrt(Cc - b * b);
    out[0] = x[0] + dt * (e0 * x[0] - Bv) + sq * a * n[0];
    out[1] = x[1] + dt * (Bv - e2 * x[1]) + sq * (b * n[0] + c * n[1]);
  } else if (model == 2) {
    out[0] = x[0] + dt * th[0] * x[0] + sq * x[0] * std::exp(0.5 * x[1]) * n[0];
    out[1] = x[1] + dt * (th[1] - std::exp(th[2]) * x[1]) + sq * std::exp(th[3]) * n[1];
  } else {
    out[0] = x[0] + dt * std::exp(th[0]) * (x[0] - x[0] * x[0] * x[0] - x[1] + th[1]) +
             sq * std::sqrt(std::exp(th[3])) * n[0];
    out[1] = x[1] + dt * (th[2] * x[0] - x[1] + 1.4) + sq * std::sqrt(std::exp(th[4])) * n[1];
  }
}

// hc_sim_step against the double step, and hc_sim_path (with and without observations, H = 0, 1, 7) against the
// step chained by hand
int check_sim(int model, int cases) {
  const int S = model == 0 ? 1 : 2, P = model == 0 ? 3 : model == 1 ? 3 : model == 2 ? 4 : 5;
  const float dt = model == 0 || model == 2 ? 1.f : 0.1f;
  int bad = 0;
  for (int c = 0; c < cases; ++c) {
    float x[2] = {0.f, 0.f}, th[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, n[2];
    for (int d = 0; d < S; ++d) x[d] = static_cast<float>(model == 1 ? uniform(50.0, 200.0) : uniform(-1.5, 1.5));
    for (int p = 0; p < P; ++p) th[p] = static_cast<float>(uniform(-0.5, 0.5));
    if (model == 1) {
      th[0] = static_cast<float>(std::log(0.5) + uniform(-0.1, 0.1));
      th[1] = static_cast<float>(std::log(0.0025) + uniform(-0.1, 0.1));
      th[2] = static_cast<float>(std::log(0.3) + uniform(-0.1, 0.1));
    }
    for (int d = 0; d < 2; ++d) n[d] = static_cast<float>(uniform(-2.0, 2.0));
    float got[2] = {0.f, 0.f};
    double ref[2] = {0.0, 0.0};
    hc_sim_step(model, x, th, dt, n, got);
    sim_step_ref(model, x, th, dt, n, ref);
    for (int d = 0; d < S; ++d)
      if (!(std::fabs(got[d] - ref[d]) <= 1e-5 * std::fmax(1.0, std::fabs(ref[d]) + std::fabs(x[d])))) {
        std::printf("sim model %d case %d coordinate %d: %.9g vs %.9g\n", model, c, d, got[d], ref[d]);
        ++bad;
      }
    for (int obs = 0; obs < (model == 2 ? 1 : 2); ++obs)
      for (int H : {0, 1, 7}) {
        const int NS = obs ? 2 * S : S;
        const size_t Hs = static_cast<size_t>(H);
        std::vector<float> nn(Hs * NS), xo(S * Hs), yo(S * Hs);
        for (float& v : nn) v = static_cast<float>(uniform(-2.0, 2.0));
        float xe[2] = {-7.f, -7.f};
        hc_sim_path(model, x, th, dt, 0.5f, H, nn.data(), xo.data(), obs ? yo.data() : nullptr, xe);
        float cur[2] = {x[0], x[1]};
        for (int t = 0; t < H; ++t) {
          float nx[2];
          const float* nt = nn.data() + static_cast<size_t>(t) * NS;
          hc_sim_step(model, cur, th, dt, nt, nx);
          for (int d = 0; d < S; ++d) {
            cur[d] = nx[d];
            const size_t at = d * Hs + t;
            const bool same = xo[at] == cur[d] && (!obs || yo[at] == cur[d] + 0.5f * nt[S + d]);
            if (!same && std::isfinite(cur[d])) { std::printf("sim path model %d H %d step %d\n", model, H, t); ++bad; }
          }
        }
        for (int d = 0; d < S; ++d)
          if (std::isfinite(cur[d]) && xe[d] != cur[d]) {
            std::printf("sim path model %d H %d: x_end\n", model, H);
            ++bad;
          }
      }
  }
  return bad;
}

// an LV row that leaves the positive orthant at its third step: NaN from there on, in x, y and x_end; a start outside
// it: NaN throughout
int check_sim_dead() {
  const float th[3] = {std::log(0.5f), std::log(0.0025f), std::log(0.3f)};
  const float x0[2] = {0.5f, 100.f};
  const int H = 6;
  std::vector<float> nn(static_cast<size_t>(H) * 4, 0.f), xo(2 * H), yo(2 * H);
  nn[2 * 4] = -30.f;  // step 2: x1 pushed far below zero
  float xe[2] = {0.f, 0.f};
  hc_sim_path(1, x0, th, 0.1f, 1.f, H, nn.data(), xo.data(), yo.data(), xe);
  int bad = 0;
  for (int d = 0; d < 2; ++d)
    for (int t = 0; t < H; ++t) {
      const bool want_nan = t >= 2;
      if (std::isnan(xo[d * H + t]) != want_nan || std::isnan(yo[d * H + t]) != want_nan) {
        std::printf("sim dead row: coordinate %d step %d: %g %g\n", d, t, xo[d * H + t], yo[d * H + t]);
        ++bad;
      }
    }
  if (!std::isnan(xe[0]) || !std::isnan(xe[1])) { std::printf("sim dead row: x_end %g %g\n", xe[0], xe[1]); ++bad; }
  const float xneg[2] = {-1.f, 100.f};
  hc_sim_path(1, xneg, th, 0.1f, 1.f, H, nn.data(), xo.data(), nullptr, xe);
  for (int i = 0; i < 2 * H; ++i)
    if (!std::isnan(xo[i])) { std::printf("sim dead start: entry %d = %g\n", i, xo[i]); ++bad; }
  return bad;
}

// Philox4x32-10 round by round from the paper: mulhi / mullo apart, the key bumped after each of the first nine rounds
void philox_ref(const uint32_t c_in[4], const uint32_t k_in[2], uint32_t out[4]) {
  uint32_t c[4] = {c_in[0], c_in[1], c_in[2], c_in[3]}, k[2] = {k_in[0], k_in[1]};
  for (int r = 0; r < 10; ++r) {
    if (r > 0) { k[0] += 0x9E3779B9u; k[1] += 0xBB67AE85u; }
    const uint64_t p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
    const uint32_t n[4] = {static_cast<uint32_t>(p1 >> 32) ^ c[1] ^ k[0], static_cast<uint32_t>(p1 & 0xFFFFFFFFull),
                           static_cast<uint32_t>(p0 >> 32) ^ c[3] ^ k[1], static_cast<uint32_t>(p0 & 0xFFFFFFFFull)};
    for (int i = 0; i < 4; ++i) c[i] = n[i];
  }
  for (int i = 0; i < 4; ++i) out[i] = c[i];
}

int check_philox() {
  struct Kat { uint32_t c[4], k[2], want[4]; };
  const Kat kats[3] = {
      {{0u, 0u, 0u, 0u}, {0u, 0u}, {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u}},
      {{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, {0xffffffffu, 0xffffffffu},
       {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu}},
      {{0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, {0xa4093822u, 0x299f31d0u},
       {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}}};
  int bad = 0;
  for (const Kat& t : kats) {
    uint32_t got[4] = {0u, 0u, 0u, 0u};
    hc_philox(t.c, t.k, got);
    if (std::memcmp(got, t.want, sizeof got) != 0) {
      std::printf("philox known answer: %08x %08x %08x %08x, want %08x %08x %08x %08x\n", got[0], got[1], got[2],
                  got[3], t.want[0], t.want[1], t.want[2], t.want[3]);
      ++bad;
    }
  }
  // random counters and keys, then the kernels' layout (group, 0, lo(row), hi(row)) with rows around 2^32
  for (int i = 0; i < 4096; ++i) {
    uint32_t c[4], k[2], got[4], ref[4];
    for (uint32_t& v : c) v = static_cast<uint32_t>(uniform(0.0, 4294967296.0));
    for (uint32_t& v : k) v = static_cast<uint32_t>(uniform(0.0, 4294967296.0));
    if (i >= 2048) {
      const uint64_t row = 0xFFFFFFFFull - 1024 + static_cast<uint64_t>(i - 2048);
      c[0] = static_cast<uint32_t>(i & 255); c[1] = 0u;
      c[2] = static_cast<uint32_t>(row); c[3] = static_cast<uint32_t>(row >> 32);
    }
    hc_philox(c, k, got);
    philox_ref(c, k, ref);
    if (std::memcmp(got, ref, sizeof got) != 0) { std::printf("philox: counter %d differs from the restatement\n", i); ++bad; }
  }
  for (uint32_t w : {0x00000000u, 0x000000FFu, 0x00000100u, 0xFFFFFEFFu, 0xFFFFFF00u, 0xFFFFFFFFu, 0x80000000u}) {
    const float want = static_cast<float>((static_cast<double>(w >> 8) + 1.0) / 16777216.0);
    const float got = hc_u01(w);
    if (got != want || !(got > 0.f) || got > 1.f) { std::printf("u01(%08x): %.9g vs %.9g\n", w, got, want); ++bad; }
  }
  return bad;
}

// The particle filter's integer half (pf_math.hpp).  Thresholds against a 128-bit restatement; systematic resampling
// against a linear count of the cumulative sums, over U = 0 and 2^24 - 1, N = 64 and 1024, a single survivor with
// W = 2^40, W one below 2^50 (every weight 2^40 but one), runs of zero weights, and weights whose cumulative sums the
// thresholds hit exactly (equal weights at U = 0: tau_j = j q = C_{j-1}); quantise on the ends of its range.
int check_pf() {
  int bad = 0;
  const uint32_t Umax = (1u << 24) - 1u;
  for (int n : {64, 1024}) {
    int l = 0;
    while ((1 << l) < n) ++l;
    std::vector<std::vector<uint64_t>> cases;
    std::vector<uint64_t> q(n, 0);
    q[n / 3] = 1ull << 40;  // a single survivor
    cases.push_back(q);
    std::fill(q.begin(), q.end(), 1ull << 40);  // W = N 2^40 (2^50 at N = 1024), every tau on a C_i at U = 0
    cases.push_back(q);
    q[n - 1] -= 1;  // one below
    cases.push_back(q);
    for (int i = 0; i < n; ++i) q[i] = (i / 7) % 2 ? 0ull : static_cast<uint64_t>(uniform(0.0, 1099511627776.0));
    q[5] = 1ull << 40;  // runs of zeros
    cases.push_back(q);
    for (int i = 0; i < n; ++i) q[i] = i < n - 3 ? 0ull : 1ull;  // W = 3, zeros first
    cases.push_back(q);
    for (int i = 0; i < n; ++i) q[i] = static_cast<uint64_t>(std::exp(uniform(-30.0, 0.0)) * 1099511627776.0);
    q[0] = 1ull << 40;
    cases.push_back(q);
    for (const auto& qc : cases)
      for (uint32_t U : {0u, 1u, Umax / 2u, Umax}) {
        std::vector<int32_t> anc(n, -1);
        std::vector<uint64_t> C(n, 0);
        const uint64_t W = hc_pf_resample(qc.data(), n, U, anc.data(), C.data());
        uint64_t sum = 0;
        for (int i = 0; i < n; ++i) {
          sum += qc[i];
          if (C[i] != sum) { std::printf("pf: cumulative sum %d\n", i); ++bad; }
        }
        if (W != sum) { std::printf("pf: W\n"); ++bad; }
        for (int j = 0; j < n; ++j) {
          const unsigned __int128 a = (static_cast<unsigned __int128>(j) << 24) + U;
          const uint64_t tau = static_cast<uint64_t>((a * W) >> (24 + l));
          if (hc_pf_threshold(static_cast<uint32_t>(j), U, W, l) != tau) { std::printf("pf: threshold %d\n", j); ++bad; }
          int want = 0;
          for (int i = 0; i < n; ++i) want += C[i] <= tau;
          if (anc[j] != want || want >= n || qc[want] == 0) {
            std::printf("pf: n %d U %u slot %d: ancestor %d, want %d\n", n, U, j, anc[j], want);
            ++bad;
          }
        }
      }
    std::vector<uint64_t> zero(n, 0), C(n, 0);
    std::vector<int32_t> anc(n, -7);
    if (hc_pf_resample(zero.data(), n, 5u, anc.data(), C.data()) != 0 || anc[0] != -7) { std::printf("pf: W = 0\n"); ++bad; }
  }
  if (hc_pf_quantise(-3.f, -3.f, 1) != (1ull << 40)) { std::printf("pf: quantise at the maximum\n"); ++bad; }
  if (hc_pf_quantise(-3.f, -3.f, 0) != 0) { std::printf("pf: quantise of a dead particle\n"); ++bad; }
  if (hc_pf_quantise(-200.f, 0.f, 1) != 0) { std::printf("pf: quantise underflow\n"); ++bad; }
  if (hc_pf_quantise(-INFINITY, -INFINITY, 1) != 0) { std::printf("pf: quantise without a finite weight\n"); ++bad; }
  if (hc_pf_quantise(-INFINITY, 0.f, 1) != 0) { std::printf("pf: quantise of -inf\n"); ++bad; }
  const uint64_t half = hc_pf_quantise(-0.6931472f, 0.f, 1);
  if (half < (1ull << 39) - (1ull << 18) || half > (1ull << 39) + (1ull << 18)) { std::printf("pf: quantise(ln 1/2)\n"); ++bad; }
  if (hc_pf_resample_u(1u, 2u, 3u) >= (1u << 24)) { std::printf("pf: U range\n"); ++bad; }
  const double li = hc_pf_ll_increment(-1.5f, 1ull << 40, 64);
  if (std::fabs(li - (-1.5 - std::log(64.0))) > 1e-12) { std::printf("pf: ll_increment %g\n", li); ++bad; }
  return bad;
}

// The particle smoother's shared math (ps_math.hpp).  The selection against a 128-bit restatement over U = 0 and
// 2^32 - 1, N = 64 and 1024, all-equal weights (W = N 2^40: 2^50 at N = 1024), one live particle, runs of zeros and
// W = 0; pair_logw plus the dropped constant against *_trans' lp; a whole draw with dead particles, with the terminal
// rule, with a NaN target and with no live particle.
int check_ps() {
  int bad = 0;
  const uint32_t Umax = 0xFFFFFFFFu;
  for (int n : {64, 1024}) {
    std::vector<std::vector<uint64_t>> cases;
    std::vector<uint64_t> q(n, 1ull << 40);  // all equal
    cases.push_back(q);
    q[n - 1] -= 1;
    cases.push_back(q);
    std::fill(q.begin(), q.end(), 0ull);
    q[n / 3] = 1ull << 40;  // one live particle
    cases.push_back(q);
    for (int i = 0; i < n; ++i) q[i] = (i / 5) % 2 ? 0ull : static_cast<uint64_t>(uniform(0.0, 1099511627776.0));
    q[7] = 1ull << 40;  // runs of zeros
    cases.push_back(q);
    for (int i = 0; i < n; ++i) q[i] = i < n - 3 ? 0ull : 1ull;  // W = 3, zeros first
    cases.push_back(q);
    for (const auto& qc : cases)
      for (uint32_t U : {0u, 1u, 0x7FFFFFFFu, 0x80000000u, Umax}) {
        uint64_t W = 0, tau = 0, sum = 0;
        const int idx = hc_ps_select(qc.data(), n, U, &W, &tau);
        for (int i = 0; i < n; ++i) sum += qc[i];
        const uint64_t want_tau = static_cast<uint64_t>((static_cast<unsigned __int128>(U) * sum) >> 32);
        int want = 0;
        uint64_t C = 0;
        for (int i = 0; i < n; ++i) {
          C += qc[i];
          want += C <= want_tau;
        }
        if (W != sum || tau != want_tau || tau >= W || hc_ps_threshold(U, sum) != want_tau || idx != want ||
            idx >= n || qc[idx] == 0) {
          std::printf("ps: n %d U %u: idx %d want %d\n", n, U, idx, want);
          ++bad;
        }
      }
    std::vector<uint64_t> zero(n, 0);
    uint64_t W = 1, tau = 1;
    if (hc_ps_select(zero.data(), n, 5u, &W, &tau) != -1 || W != 0) { std::printf("ps: W = 0\n"); ++bad; }
  }
  if (hc_ps_threshold(Umax, 1ull << 50) != (1ull << 50) - (1ull << 18)) { std::printf("ps: threshold at 2^50\n"); ++bad; }
  // pair_logw + the dropped constant = *_trans' lp
  const float ths[4][5] = {{5.f, 0.5f, 1.0986123f, 0.f, 0.f}, {-0.6931472f, -5.9914646f, -1.2039728f, 0.f, 0.f},
                           {0.f, 0.f, 0.f, 0.f, 0.f}, {0.6931472f, 1.f, 1.5f, -0.6931472f, -1.2039728f}};
  const float dts[4] = {1.f, 0.1f, 0.1f, 0.1f};
  for (int model : {0, 1, 3})
    for (int rep = 0; rep < 200; ++rep) {
      float x[2], xt[2];
      for (int d = 0; d < 2; ++d) {
        const double c = model == 0 ? 10.0 : model == 1 ? 100.0 : 1.0;
        x[d] = static_cast<float>(c * uniform(0.5, 1.5));
        xt[d] = static_cast<float>(x[d] + (model == 1 ? 5.0 : model == 0 ? 6.0 : 0.3) * uniform(-1.0, 1.0));
      }
      float dropped = 0.f;
      const float lw = hc_ps_pair_logw(model, x, xt, ths[model], dts[model], &dropped);
      const float lp = lp_of(model, x, xt, ths[model], dts[model]);
      if (!std::isfinite(lw) || std::fabs((lw + dropped) - lp) > 2e-5f * std::fmax(1.f, std::fabs(lp))) {
        std::printf("ps: model %d pair_logw %.9g + %.9g vs lp %.9g\n", model, lw, dropped, lp);
        ++bad;
      }
    }
  // a whole draw: LV, 64 particles, every fourth dead (NaN or outside the orthant)
  {
    const int n = 64;
    std::vector<float> x(2 * n);
    for (int i = 0; i < n; ++i) {
      x[2 * i] = static_cast<float>(100.0 * uniform(0.9, 1.1));
      x[2 * i + 1] = static_cast<float>(100.0 * uniform(0.9, 1.1));
      if (i % 4 == 1) x[2 * i] = i % 8 == 1 ? NAN : -1.f;
    }
    const float xt[2] = {101.f, 99.f}, nan_t[2] = {NAN, 99.f};
    std::vector<uint64_t> q(n, 7);
    float m = 0.f;
    for (uint32_t U : {0u, 0x12345678u, Umax}) {
      int idx = hc_ps_draw(1, x.data(), n, ths[1], 0.1f, xt, U, q.data(), &m);
      uint64_t top = 0;
      for (int i = 0; i < n; ++i) {
        if (i % 4 == 1 && q[i] != 0) { std::printf("ps: a dead particle has weight\n"); ++bad; }
        top = std::max(top, q[i]);
      }
      if (idx < 0 || idx >= n || idx % 4 == 1 || q[idx] == 0 || top != (1ull << 40) || !std::isfinite(m)) {
        std::printf("ps: draw U %u idx %d\n", U, idx);
        ++bad;
      }
      idx = hc_ps_draw(1, x.data(), n, ths[1], 0.1f, nullptr, U, q.data(), &m);  // terminal: uniform over the live
      for (int i = 0; i < n; ++i)
        if (q[i] != (i % 4 == 1 ? 0ull : 1ull << 40)) { std::printf("ps: terminal weight %d\n", i); ++bad; }
      if (idx < 0 || idx % 4 == 1 || m != 0.f) { std::printf("ps: terminal draw idx %d\n", idx); ++bad; }
      if (hc_ps_draw(1, x.data(), n, ths[1], 0.1f, nan_t, U, q.data(), &m) != -1) { std::printf("ps: NaN target\n"); ++bad; }
    }
    for (int i = 0; i < n; ++i) x[2 * i + 1] = -2.f;  // no live particle
    if (hc_ps_draw(1, x.data(), n, ths[1], 0.1f, xt, 9u, q.data(), &m) != -1 ||
        hc_ps_draw(1, x.data(), n, ths[1], 0.1f, nullptr, 9u, q.data(), &m) != -1) {
      std::printf("ps: no live particle\n");
      ++bad;
    }
  }
  if (hc_ps_select_u(1u, 2u, 3u) == hc_ps_select_u(1u, 3u, 3u)) { std::printf("ps: select_u\n"); ++bad; }
  return bad;
}

// gp_math.hpp against the general formulas in double: S = Sigma_OO + R I, logw = log N(y_O; mu_O, S),
// K = Sigma_.O S^-1, m = mu + K (y_O - mu_O), P = Sigma - K Sigma_O. = L L^T
int check_gp() {
  int bad = 0;
  const float ths[4][5] = {{5.f, 0.5f, 1.0986123f, 0.f, 0.f}, {-0.6931472f, -5.9914646f, -1.2039728f, 0.f, 0.f},
                           {0.f, 0.f, 0.f, 0.f, 0.f}, {0.6931472f, 1.f, 1.5f, -0.6931472f, -1.2039728f}};
  const float dts[4] = {1.f, 0.1f, 0.1f, 0.1f};
  const float masks[3][2] = {{1.f, 1.f}, {1.f, 0.f}, {0.f, 1.f}};
  for (int model : {0, 1, 3}) {
    const int S = model == 0 ? 1 : 2;
    for (int mk = 0; mk < (S == 1 ? 1 : 3); ++mk)
      for (double rel : {0.05, 0.5, 1.0, 30.0, 1000.0})
        for (int rep = 0; rep < 40; ++rep) {
          float x[2], y[2], n[2], mo[6], co[5], out[2];
          const double c = model == 0 ? 10.0 : model == 1 ? 100.0 : 1.0;
          for (int d = 0; d < 2; ++d) {
            x[d] = static_cast<float>(c * uniform(0.5, 1.5));
            n[d] = static_cast<float>(uniform(-2.0, 2.0));
          }
          hc_gp_moments(model, x, ths[model], dts[model], mo);
          const double mu[2] = {mo[0], mo[1]}, Sg[2][2] = {{mo[2], mo[3]}, {mo[3], mo[4]}};
          const float* bin = S == 1 ? masks[1] : masks[mk];
          const double sd0 = std::sqrt(bin[0] != 0.f ? Sg[0][0] : Sg[1][1]);
          const float obs_std = static_cast<float>(rel * sd0);
          const float Rf = obs_std * obs_std;
          const double R = Rf;
          for (int d = 0; d < 2; ++d)  // an unobserved coordinate's y is a filler that must not be read
            y[d] = bin[d] != 0.f ? static_cast<float>(mu[d] + std::sqrt(Sg[d][d] + R) * uniform(-2.0, 2.0)) : NAN;
          int O[2], no = 0;
          for (int d = 0; d < S; ++d)
            if (bin[d] != 0.f) O[no++] = d;
          double Sm[2][2] = {{1.0, 0.0}, {0.0, 1.0}}, r[2] = {0.0, 0.0};
          for (int a = 0; a < no; ++a) {
            r[a] = y[O[a]] - mu[O[a]];
            for (int b = 0; b < no; ++b) Sm[a][b] = Sg[O[a]][O[b]] + (a == b ? R : 0.0);
          }
          const double det = Sm[0][0] * Sm[1][1] - Sm[0][1] * Sm[1][0];
          const double Si[2][2] = {{Sm[1][1] / det, -Sm[0][1] / det}, {-Sm[1][0] / det, Sm[0][0] / det}};
          double quad = 0.0;
          for (int a = 0; a < no; ++a)
            for (int b = 0; b < no; ++b) quad += r[a] * Si[a][b] * r[b];
          const double lw = -0.5 * quad - 0.5 * std::log(det) - 0.5 * no * std::log(2.0 * M_PI);
          double K[2][2] = {{0.0, 0.0}, {0.0, 0.0}}, m[2], P[2][2];
          for (int d = 0; d < S; ++d)
            for (int a = 0; a < no; ++a)
              for (int b = 0; b < no; ++b) K[d][a] += Sg[d][O[b]] * Si[b][a];
          for (int d = 0; d < S; ++d) {
            m[d] = mu[d];
            for (int a = 0; a < no; ++a) m[d] += K[d][a] * r[a];
            for (int e = 0; e < S; ++e) {
              P[d][e] = Sg[d][e];
              for (int a = 0; a < no; ++a) P[d][e] -= K[d][a] * Sg[O[a]][e];
            }
          }
          const float got = hc_gp_logw(model, x, ths[model], dts[model], y, bin, Rf);
          hc_gp_cond(model, x, ths[model], dts[model], y, bin, Rf, co);
          hc_gp_step(model, x, ths[model], dts[model], y, bin, Rf, n, out);
          bool ok = std::isfinite(got) && std::fabs(got - lw) <= 2e-5 * std::fmax(1.0, std::fabs(lw));
          for (int d = 0; d < S; ++d) ok = ok && std::fabs(co[d] - m[d]) <= 2e-5 * std::fmax(1.0, std::fabs(m[d]));
          // L L^T = P to fp32 rounding of Sigma's entries (P itself cancels at small R)
          const double ll[2][2] = {{double(co[2]) * co[2], double(co[2]) * co[3]},
                                   {double(co[2]) * co[3], double(co[3]) * co[3] + double(co[4]) * co[4]}};
          for (int d = 0; d < S; ++d)
            for (int e = 0; e < S; ++e)
              ok = ok && std::fabs(ll[d][e] - P[d][e]) <= 2e-5 * std::sqrt(Sg[d][d] * Sg[e][e]);
          ok = ok && out[0] == co[0] + co[2] * n[0];
          if (S == 2) ok = ok && std::fabs(out[1] - (co[1] + (co[3] * n[0] + co[4] * n[1]))) <= 1e-5 * std::fabs(co[1]);
          if (!ok) {
            std::printf("gp: model %d mask %d rel %g: logw %.9g vs %.9g, m %.9g %.9g vs %.9g %.9g\n", model, mk, rel, got,
                        lw, co[0], co[1], m[0], S == 2 ? m[1] : 0.0);
            ++bad;
          }
        }
  }
  // the clamp: a radicand that rounds negative gives 0, a NaN one stays NaN
  if (hc_gp_l11(1.f, 1.0000001f) != 0.f || hc_gp_l11(4.f, 0.f) != 2.f || !std::isnan(hc_gp_l11(NAN, 1.f))) {
    std::printf("gp: clamp\n");
    ++bad;
  }
  // whole steps: LV, 64 particles, every fourth dead
  {
    const int n = 64;
    std::vector<float> x(2 * n), nn(2 * n), xo(2 * n);
    for (int i = 0; i < n; ++i) {
      x[2 * i] = static_cast<float>(100.0 * uniform(0.9, 1.1));
      x[2 * i + 1] = static_cast<float>(100.0 * uniform(0.9, 1.1));
      if (i % 4 == 1) x[2 * i] = i % 8 == 1 ? NAN : -1.f;
      nn[2 * i] = static_cast<float>(uniform(-2.0, 2.0));
      nn[2 * i + 1] = static_cast<float>(uniform(-2.0, 2.0));
    }
    std::vector<uint64_t> q(n), C(n);
    std::vector<int32_t> anc(n);
    const float y[2] = {101.f, 99.f}, none[2] = {0.f, 0.f};
    float m = 0.f;
    for (int mk = 0; mk < 3; ++mk) {
      const uint64_t W = hc_gp_filter_step(1, x.data(), n, ths[1], 0.1f, y, masks[mk], 1.f, nn.data(), 0x654321u,
                                           xo.data(), q.data(), anc.data(), C.data(), &m);
      uint64_t top = 0;
      for (int i = 0; i < n; ++i) {
        top = std::max(top, q[i]);
        if (i % 4 == 1 && q[i] != 0) { std::printf("gp: a dead particle has weight\n"); ++bad; }
        if (anc[i] < 0 || anc[i] >= n || q[anc[i]] == 0 || !std::isfinite(xo[2 * i]) || !std::isfinite(xo[2 * i + 1])) {
          std::printf("gp: slot %d ancestor %d\n", i, anc[i]);
          ++bad;
        }
      }
      if (W == 0 || top != (1ull << 40) || !std::isfinite(m)) { std::printf("gp: step mask %d\n", mk); ++bad; }
    }
    // unobserved: sim::advance, slot for slot
    hc_gp_filter_step(1, x.data(), n, ths[1], 0.1f, y, none, 1.f, nn.data(), 0u, xo.data(), q.data(), anc.data(),
                      C.data(), &m);
    for (int i = 0; i < n; ++i) {
      float xp[2], xe[2];
      hc_sim_path(1, &x[2 * i], ths[1], 0.1f, 0.f, 1, &nn[2 * i], xp, nullptr, xe);
      if (std::memcmp(xe, &xo[2 * i], 8) != 0 && !(std::isnan(xe[0]) && std::isnan(xo[2 * i]))) {
        std::printf("gp: unobserved step %d\n", i);
        ++bad;
      }
    }
    for (int i = 0; i < n; ++i) x[2 * i + 1] = -2.f;  // no live particle
    if (hc_gp_filter_step(1, x.data(), n, ths[1], 0.1f, y, masks[0], 1.f, nn.data(), 9u, xo.data(), q.data(),
                          anc.data(), C.data(), &m) != 0 || !std::isnan(xo[0]) || !std::isnan(xo[2 * n - 1])) {
      std::printf("gp: no live particle\n");
      ++bad;
    }
  }
  return bad;
}

// svf_math.hpp: the weight against a double restatement; the move against hc_sim_step's second coordinate, bit for
// bit; pair_logw plus the dropped constant against sv_trans' lp of the joint step (y_next, h) -> (y_next2, xt), which
// factorises into the transition of h and the weight; whole serial filter steps and backward draws with dead
// particles, a NaN target, the terminal rule, no live particle and y_prev = 0.
int check_svf() {
  int bad = 0;
  for (float dt : {1.f, 0.1f})
    for (int rep = 0; rep < 400; ++rep) {
      float th[5] = {0.001f, -0.6f, -2.5257287f, -0.6931472f, 0.f};
      for (int i = 0; i < 4; ++i) th[i] += static_cast<float>(uniform(-0.2, 0.2));
      const float h = static_cast<float>(uniform(-12.0, -3.0));
      const float y0 = static_cast<float>(uniform(1.0, 15.0) * (uniform(0.0, 1.0) < 0.5 ? -1.0 : 1.0));
      const double sd = std::sqrt(static_cast<double>(dt)) * std::fabs(y0) * std::exp(0.5 * h);
      const float y1 = static_cast<float>(y0 + sd * uniform(-3.0, 3.0));
      const float n = static_cast<float>(uniform(-3.0, 3.0));
      const double r = static_cast<double>(y1) - y0 - static_cast<double>(dt) * th[0] * y0;
      const double want = -0.5 * std::log(2.0 * M_PI) - std::log(std::sqrt(static_cast<double>(dt)) * std::fabs(y0)) -
                          0.5 * h - 0.5 * r * r / (dt * static_cast<double>(y0) * y0 * std::exp(static_cast<double>(h)));
      const float lw = hc_svf_logw(h, y0, y1, th, dt);
      // (r cancels two nearby floats: the bar is the relative rounding of y1 - y0 carried into r^2 / var)
      const double rel = 4e-7 * (std::fabs(y1) + std::fabs(y0)) / std::fmax(std::fabs(r), 1e-30);
      if (!std::isfinite(lw) || std::fabs(lw - want) > 2e-5 * std::fmax(1.0, std::fabs(want)) +
                                                           rel * r * r / (sd * sd)) {
        std::printf("svf: logw %.9g vs %.9g\n", lw, want);
        ++bad;
      }
      const float x[2] = {y0, h}, nn[2] = {static_cast<float>(uniform(-2.0, 2.0)), n};
      float out[2];
      hc_sim_step(2, x, th, dt, nn, out);
      const float mv = hc_svf_move(h, th, dt, n);
      if (to_bits(mv) != to_bits(out[1])) { std::printf("svf: move %.9g vs em_step %.9g\n", mv, out[1]); ++bad; }
      const float xt = out[1];
      const float xh[2] = {y0, h}, xn[2] = {y1, xt};
      float dropped = 0.f;
      const float pw = hc_svf_pair_logw(h, xt, y0, y1, th, dt, &dropped);
      const float lp = lp_of(2, xh, xn, th, dt);
      if (!std::isfinite(pw) || std::fabs((pw + dropped) - lp) > 4e-5f * std::fmax(1.f, std::fabs(lp)) +
                                                                     static_cast<float>(rel * r * r / (sd * sd))) {
        std::printf("svf: pair_logw %.9g + %.9g vs lp %.9g\n", pw, dropped, lp);
        ++bad;
      }
    }
  const float th[5] = {0.001f, -0.6f, -2.5257287f, -0.6931472f, 0.f};
  if (hc_svf_logw(NAN, 1.f, 1.1f, th, 1.f) != -INFINITY || hc_svf_logw(INFINITY, 1.f, 1.1f, th, 1.f) != -INFINITY ||
      !std::isnan(hc_svf_move(NAN, th, 1.f, 0.f)) || !std::isnan(hc_svf_move(-INFINITY, th, 1.f, 0.f))) {
    std::printf("svf: dead particle\n");
    ++bad;
  }
  for (int n : {64, 1024}) {
    std::vector<float> h(n), nn(n), ho(n);
    for (int i = 0; i < n; ++i) {
      h[i] = i % 4 == 1 ? NAN : static_cast<float>(uniform(-10.0, -6.0));
      nn[i] = static_cast<float>(uniform(-2.0, 2.0));
    }
    std::vector<uint64_t> q(n), C(n);
    std::vector<int32_t> anc(n);
    float m = 0.f;
    uint64_t W = hc_svf_filter_step(h.data(), n, th, 1.f, 5.25f, 5.31f, nn.data(), 0x654321u, ho.data(), q.data(),
                                    anc.data(), C.data(), &m);
    uint64_t top = 0;
    for (int i = 0; i < n; ++i) {
      top = std::max(top, q[i]);
      if (i % 4 == 1 && q[i] != 0) { std::printf("svf: a dead particle has weight\n"); ++bad; }
      if (anc[i] < 0 || anc[i] >= n || q[anc[i]] == 0 || to_bits(ho[i]) != to_bits(hc_svf_move(h[anc[i]], th, 1.f, nn[i]))) {
        std::printf("svf: slot %d ancestor %d\n", i, anc[i]);
        ++bad;
      }
    }
    if (W == 0 || top != (1ull << 40) || !std::isfinite(m)) { std::printf("svf: filter step\n"); ++bad; }
    if (hc_svf_filter_step(h.data(), n, th, 1.f, 0.f, 5.31f, nn.data(), 1u, ho.data(), q.data(), anc.data(), C.data(),
                           &m) != 0 || !std::isnan(ho[0])) {
      std::printf("svf: y_prev = 0\n");
      ++bad;
    }
    for (uint32_t U : {0u, 0x12345678u, 0xFFFFFFFFu}) {
      int idx = hc_svf_draw(h.data(), n, th, 1.f, 1, -8.3f, 5.25f, 5.31f, U, q.data(), &m);
      top = 0;
      for (int i = 0; i < n; ++i) {
        top = std::max(top, q[i]);
        if (i % 4 == 1 && q[i] != 0) { std::printf("svf: a dead particle is drawn\n"); ++bad; }
      }
      if (idx < 0 || idx >= n || idx % 4 == 1 || q[idx] == 0 || top != (1ull << 40)) { std::printf("svf: draw\n"); ++bad; }
      idx = hc_svf_draw(h.data(), n, th, 1.f, 0, 0.f, 0.f, 0.f, U, q.data(), &m);
      for (int i = 0; i < n; ++i)
        if (q[i] != (i % 4 == 1 ? 0ull : 1ull << 40)) { std::printf("svf: terminal weight %d\n", i); ++bad; }
      if (idx < 0 || idx % 4 == 1 || m != 0.f) { std::printf("svf: terminal draw\n"); ++bad; }
      if (hc_svf_draw(h.data(), n, th, 1.f, 1, NAN, 5.25f, 5.31f, U, q.data(), &m) != -1) { std::printf("svf: NaN target\n"); ++bad; }
    }
    std::fill(h.begin(), h.end(), NAN);
    if (hc_svf_filter_step(h.data(), n, th, 1.f, 5.25f, 5.31f, nn.data(), 1u, ho.data(), q.data(), anc.data(), C.data(),
                           &m) != 0 || !std::isnan(ho[n - 1]) ||
        hc_svf_draw(h.data(), n, th, 1.f, 1, -8.f, 5.25f, 5.31f, 9u, q.data(), &m) != -1 ||
        hc_svf_draw(h.data(), n, th, 1.f, 0, 0.f, 0.f, 0.f, 9u, q.data(), &m) != -1) {
      std::printf("svf: no live particle\n");
      ++bad;
    }
  }
  return bad;
}

// mh_math.hpp: the words are Philox on counter (g, 2, lo(r), hi(r)); u stays inside (0, 1); a zero factor proposes
// theta itself and L = I adds the normals; the log-prior of the mean is 0; the decision's -inf and NaN cases
int check_mh() {
  int bad = 0;
  const uint64_t seed = 0x0123456789ABCDEFull, r = hc_mh_row(0xFFFFFFF0ull, 3, 5, 2, 64);
  if (r != 0xFFFFFFF0ull + (3 * 5 + 2) * 64) { std::printf("mh: row\n"); ++bad; }
  for (uint32_t g = 0; g < 3; ++g) {
    const uint32_t ctr[4] = {g, 2u, static_cast<uint32_t>(r), static_cast<uint32_t>(r >> 32)};
    const uint32_t key[2] = {static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32)};
    uint32_t got[4], want[4];
    hc_mh_words(g, r, seed, got);
    hc_philox(ctr, key, want);
    if (std::memcmp(got, want, sizeof got) != 0) { std::printf("mh: words of group %u\n", g); ++bad; }
  }
  for (uint32_t w : {0x00000000u, 0x000000FFu, 0x00000100u, 0xFFFFFF00u, 0xFFFFFFFFu}) {
    const double u = hc_mh_uniform(w), lu = hc_mh_log_uniform(w);
    if (!(u > 0.0 && u < 1.0) || u != (static_cast<double>(w >> 8) + 0.5) / 16777216.0 || !(lu < 0.0) ||
        !std::isfinite(lu)) {
      std::printf("mh: uniform(%08x) = %.17g\n", w, u);
      ++bad;
    }
  }
  float xi[8];
  hc_mh_xi(r, seed, xi);
  for (float v : xi)
    if (!std::isfinite(v) || std::fabs(v) > 6.f) { std::printf("mh: xi %g\n", v); ++bad; }
  for (int P : {3, 5}) {
    std::vector<float> L(static_cast<size_t>(P) * P, 0.f), th(P), out(P), prior(2 * static_cast<size_t>(P));
    for (int p = 0; p < P; ++p) {
      th[p] = static_cast<float>(uniform(-2.0, 2.0));
      prior[2 * p] = th[p];
      prior[2 * p + 1] = 0.5f;
    }
    hc_mh_propose(th.data(), L.data(), xi, P, out.data());
    for (int p = 0; p < P; ++p)
      if (out[p] != th[p]) { std::printf("mh: zero factor\n"); ++bad; }
    for (int p = 0; p < P; ++p) L[static_cast<size_t>(p) * P + p] = 1.f;
    hc_mh_propose(th.data(), L.data(), xi, P, out.data());
    for (int p = 0; p < P; ++p)
      if (out[p] != static_cast<float>(static_cast<double>(th[p]) + xi[p])) { std::printf("mh: unit factor\n"); ++bad; }
    if (hc_mh_log_prior(th.data(), prior.data(), P) != 0.0) { std::printf("mh: log-prior at the mean\n"); ++bad; }
    prior[0] = th[0] - 1.f;
    if (hc_mh_log_prior(th.data(), prior.data(), P) != -2.0) { std::printf("mh: log-prior two sd away\n"); ++bad; }
  }
  const double inf = INFINITY;
  if (hc_mh_accept(-1.0, -inf, -3.0, 0.0, 0.0) != 0 || hc_mh_accept(-1.0, -3.0, -inf, 0.0, 0.0) != 1 ||
      hc_mh_accept(-1.0, -inf, -inf, 0.0, 0.0) != 0 || hc_mh_accept(-1.0, -3.0, -3.0, -0.5, 0.0) != 1 ||
      hc_mh_accept(-0.5, -3.0, -3.0, -0.5, 0.0) != 0 || hc_mh_accept(-1.0, NAN, -3.0, 0.0, 0.0) != 0) {
    std::printf("mh: decision\n");
    ++bad;
  }
  return bad;
}

// mh::adapt (the adaptive chain's factor update): an update and a downdate at P = 3, 4, 5 reproduce
// L (I + d xi xi^T / |xi|^2) L^T to the fp32 rounding of the factor and keep a positive diagonal; a downdate that
// reaches r2 <= 0, a diagonal that underflows in fp32 and xi = 0 hand the input back untouched; alpha and eta at
// their corners
int check_mh_adapt() {
  int bad = 0;
  for (int P : {3, 4, 5}) {
    for (double alpha : {1.0, 0.0}) {
      std::vector<float> L(static_cast<size_t>(P) * P, 0.f), L0, xi(8);
      for (int p = 0; p < P; ++p) {
        for (int j = 0; j < p; ++j) L[static_cast<size_t>(p) * P + j] = static_cast<float>(uniform(-0.5, 0.5));
        L[static_cast<size_t>(p) * P + p] = static_cast<float>(uniform(0.5, 1.5));
      }
      for (float& x : xi) x = static_cast<float>(uniform(-2.0, 2.0));
      L0 = L;
      const double eta = 0.7, d = eta * (alpha - 0.234);
      if (hc_mh_adapt(L.data(), xi.data(), alpha, eta, 0.234, P) != 1) { std::printf("adapt: P=%d kept\n", P); ++bad; }
      double n2 = 0.0, big = 0.0, err = 0.0;
      std::vector<double> w(P);
      for (int j = 0; j < P; ++j) n2 += static_cast<double>(xi[j]) * xi[j];
      for (int p = 0; p < P; ++p) {
        w[p] = 0.0;
        for (int j = 0; j <= p; ++j) w[p] += static_cast<double>(L0[static_cast<size_t>(p) * P + j]) * xi[j];
      }
      for (int p = 0; p < P; ++p) {
        if (!(L[static_cast<size_t>(p) * P + p] > 0.f)) { std::printf("adapt: diagonal\n"); ++bad; }
        for (int q = 0; q < P; ++q) {
          double got = 0.0, want = d * w[p] * w[q] / n2;
          for (int j = 0; j < P; ++j) {
            got += static_cast<double>(L[static_cast<size_t>(p) * P + j]) * L[static_cast<size_t>(q) * P + j];
            want += static_cast<double>(L0[static_cast<size_t>(p) * P + j]) * L0[static_cast<size_t>(q) * P + j];
          }
          big = std::fmax(big, std::fabs(want));
          err = std::fmax(err, std::fabs(got - want));
          if (q > p && L[static_cast<size_t>(p) * P + q] != 0.f) { std::printf("adapt: upper part\n"); ++bad; }
        }
      }
      if (!(err <= 1e-6 * big)) { std::printf("adapt: P=%d alpha=%g identity %g of %g\n", P, alpha, err, big); ++bad; }
      // xi = 0: nothing to do
      std::vector<float> zero(8, 0.f), keep = L;
      if (hc_mh_adapt(L.data(), zero.data(), alpha, eta, 0.234, P) != 0 ||
          std::memcmp(L.data(), keep.data(), L.size() * sizeof(float)) != 0) {
        std::printf("adapt: xi = 0\n");
        ++bad;
      }
    }
    // a downdate with |d| > 1 along e_0 (outside the kernel's range, the guard's own case): r2 <= 0 at k = 0
    {
      std::vector<float> L(static_cast<size_t>(P) * P, 0.f), xi(8, 0.f);
      for (int p = 0; p < P; ++p) L[static_cast<size_t>(p) * P + p] = 1.f;
      xi[0] = 1.f;
      const std::vector<float> keep = L;
      if (hc_mh_adapt(L.data(), xi.data(), 0.0, 8.0, 0.5, P) != 0 ||
          std::memcmp(L.data(), keep.data(), L.size() * sizeof(float)) != 0) {
        std::printf("adapt: r2 <= 0\n");
        ++bad;
      }
    }
    // a diagonal of the smallest subnormal, quartered by the downdate: rounds to 0 in fp32
    {
      std::vector<float> L(static_cast<size_t>(P) * P, 0.f), xi(8, 0.f);
      for (int p = 0; p < P; ++p) L[static_cast<size_t>(p) * P + p] = 1.f;
      L[0] = 1.4e-45f;
      xi[0] = 1.f;
      const std::vector<float> keep = L;
      if (hc_mh_adapt(L.data(), xi.data(), 0.0, 1.0, 0.9375, P) != 0 ||
          std::memcmp(L.data(), keep.data(), L.size() * sizeof(float)) != 0) {
        std::printf("adapt: fp32 underflow\n");
        ++bad;
      }
    }
  }
  const double inf = INFINITY;
  if (hc_mh_alpha(NAN, -3.0, 0.0, 0.0) != 0.0 || hc_mh_alpha(-inf, -inf, 0.0, 0.0) != 0.0 ||
      hc_mh_alpha(-3.0, -inf, 0.0, 0.0) != 1.0 || hc_mh_alpha(-3.0, -3.0, 0.0, 0.0) != 1.0 ||
      hc_mh_alpha(-inf, -3.0, 0.0, 0.0) != 0.0 || hc_mh_alpha(-4.0, -3.0, 0.0, 0.0) != std::exp(-1.0)) {
    std::printf("adapt: alpha\n");
    ++bad;
  }
  if (hc_mh_eta(3, 0, 0.5) != 1.0 || hc_mh_eta(3, 7, 0.5) != 1.0 || !(hc_mh_eta(3, 9, 0.5) < 1.0) ||
      hc_mh_eta(4, 3, 1.0) != 1.0 || std::fabs(hc_mh_eta(4, 4, 1.0) - 0.8) > 1e-15) {
    std::printf("adapt: eta\n");
    ++bad;
  }
  return bad;
}

// hc_svpmmh_iteration: with a zero factor the proposal is theta itself and lp' = lp; ll' is the sum of the traced
// increments; every traced ancestor is in range and every new state the move of its ancestor's; a chain at -inf accepts
// a live proposal; a zero in the series, a start that is not finite and T = 0 behave as the kernel's text says
int check_svpmmh() {
  int bad = 0;
  const uint64_t seed = 0x0BADC0FFEE123457ull;
  const float th[4] = {0.001f, -0.6f, -2.5257287f, -0.6931472f};
  const float prior[8] = {0.001f, 0.05f, -0.6f, 0.2f, -2.5f, 0.3f, -0.7f, 0.3f};
  for (int n : {64, 128}) {
    for (int T : {0, 1, 5, 9}) {
      std::vector<float> y(static_cast<size_t>(T) + 1), L(16, 0.f), h_tr(static_cast<size_t>(T + 1) * n),
          n_tr(static_cast<size_t>(T) * n + 1), m_tr(T + 1);
      std::vector<uint64_t> q_tr(static_cast<size_t>(T) * n + 1), W_tr(T + 1);
      std::vector<int32_t> anc_tr(static_cast<size_t>(T) * n + 1);
      y[0] = 5.f;
      for (int t = 0; t < T; ++t) y[t + 1] = y[t] * (1.f + 0.02f * static_cast<float>(uniform(-1.0, 1.0)));
      float thp[4];
      double out[4];
      int acc = hc_svpmmh_iteration(seed, 1000, 3, 5, 2, n, T, 1.f, th, -INFINITY, L.data(), prior, -8.5f, y.data(), thp,
                                    out, h_tr.data(), q_tr.data(), anc_tr.data(), n_tr.data(), m_tr.data(), W_tr.data());
      if (std::memcmp(thp, th, sizeof thp) != 0 || out[0] != out[1]) { std::printf("svpmmh: zero factor\n"); ++bad; }
      if (!(out[2] < 0.0) || !std::isfinite(out[3]) || acc != 1) {
        std::printf("svpmmh: n=%d T=%d ll'=%g acc=%d\n", n, T, out[3], acc);
        ++bad;
      }
      double ll = 0.0;
      for (int t = 0; t < T; ++t) {
        ll += static_cast<double>(m_tr[t]) + std::log(static_cast<double>(W_tr[t])) - 40.0 * std::log(2.0) -
              std::log(static_cast<double>(n));
        for (int p = 0; p < n; ++p) {
          const size_t o = static_cast<size_t>(t) * n;
          const int a = anc_tr[o + p];
          if (a < 0 || a >= n) { std::printf("svpmmh: ancestor %d\n", a); ++bad; continue; }
          const float want = hc_svf_move(h_tr[o + a], thp, 1.f, n_tr[o + p]);
          if (std::memcmp(&want, &h_tr[o + n + p], sizeof want) != 0) { std::printf("svpmmh: move\n"); ++bad; }
        }
      }
      if (std::fabs(ll - out[3]) > 1e-9) { std::printf("svpmmh: ll' %.17g against %.17g\n", out[3], ll); ++bad; }
      // against itself the same finite proposal is accepted iff log u < 0: always
      if (hc_svpmmh_iteration(seed, 1000, 3, 5, 2, n, T, 1.f, th, out[3], L.data(), prior, -8.5f, y.data(), thp, out,
                              nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != 1) {
        std::printf("svpmmh: equal estimates\n");
        ++bad;
      }
      if (T >= 5) {
        y[2] = 0.f;  // step 2 divides by it: NaN weights, W = 0
        acc = hc_svpmmh_iteration(seed, 1000, 3, 5, 2, n, T, 1.f, th, -3.0, L.data(), prior, -8.5f, y.data(), thp, out,
                                  nullptr, nullptr, nullptr, nullptr, nullptr, W_tr.data());
        if (acc != 0 || out[3] != -INFINITY || W_tr[2] != 0) { std::printf("svpmmh: a zero in y\n"); ++bad; }
      }
      if (T >= 1) {
        acc = hc_svpmmh_iteration(seed, 1000, 3, 5, 2, n, T, 1.f, th, -INFINITY, L.data(), prior, NAN, y.data(), thp, out,
                                  nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        if (acc != 0 || out[3] != -INFINITY) { std::printf("svpmmh: a NaN start\n"); ++bad; }
      }
    }
  }
  return bad;
}

// cpm_math.hpp: cn is rho u + sigma eps with each product rounded on its own; sigma^2 + rho^2 = 1; the sort key's
// unsigned order is the numeric order with -0 before +0 and everything not finite last, key_value inverts it; the
// resampling integer is monotone, clamped at both ends and half of 2^24 at 0
int check_cpm() {
  int bad = 0;
  for (float rho : {0.f, 0.5f, 0.9f, 0.99f, 0.999f, 0.9999f}) {
    const float s = hc_cpm_sigma(rho);
    if (std::fabs(static_cast<double>(s) * s + static_cast<double>(rho) * rho - 1.0) > 2e-7 || !hc_cpm_valid_rho(rho)) {
      std::printf("cpm: sigma(%g) = %g\n", rho, s);
      ++bad;
    }
    for (int i = 0; i < 200; ++i) {
      const float u = static_cast<float>(uniform(-4.0, 4.0)), e = static_cast<float>(uniform(-4.0, 4.0));
      volatile float a = rho * u, b = s * e;
      const float want = a + b, got = hc_cpm_cn(u, e, rho, s);
      if (std::memcmp(&want, &got, sizeof want) != 0) { std::printf("cpm: cn(%g, %g)\n", u, e); ++bad; }
    }
  }
  if (hc_cpm_valid_rho(1.f) || hc_cpm_valid_rho(-0.1f) || hc_cpm_valid_rho(NAN)) { std::printf("cpm: rho\n"); ++bad; }
  const float inf = INFINITY;
  const float asc[] = {-3.4e38f, -8.5f, -1e-40f, -0.f, 0.f, 1e-40f, 1.f, 3.4e38f};
  for (size_t i = 0; i < sizeof asc / sizeof asc[0]; ++i) {
    const uint32_t k = hc_cpm_sort_key(asc[i]);
    const float back = hc_cpm_key_value(k);
    if (std::memcmp(&back, &asc[i], sizeof back) != 0) { std::printf("cpm: key_value(key(%g))\n", asc[i]); ++bad; }
    if (i && !(hc_cpm_sort_key(asc[i - 1]) < k)) { std::printf("cpm: key order at %g\n", asc[i]); ++bad; }
    if (k == 0xFFFFFFFFu) { std::printf("cpm: a finite value has the dead key\n"); ++bad; }
  }
  for (float v : {inf, -inf, NAN, -NAN}) {
    if (hc_cpm_sort_key(v) != 0xFFFFFFFFu) { std::printf("cpm: key of %g\n", v); ++bad; }
  }
  if (!std::isnan(hc_cpm_key_value(0xFFFFFFFFu))) { std::printf("cpm: the dead key's value\n"); ++bad; }
  if (hc_cpm_resample_u(0.f) != (1u << 23) || hc_cpm_resample_u(-40.f) != 0u || hc_cpm_resample_u(40.f) != 16777215u ||
      hc_cpm_resample_u(8.f) != 16777215u || hc_cpm_resample_u(-inf) != 0u || hc_cpm_resample_u(inf) != 16777215u) {
    std::printf("cpm: resample_u ends\n");
    ++bad;
  }
  uint32_t last = 0;
  for (int i = -800; i <= 800; ++i) {
    const uint32_t U = hc_cpm_resample_u(0.01f * i);
    if (U < last || U > 16777215u) { std::printf("cpm: resample_u(%g) = %u\n", 0.01 * i, U); ++bad; }
    last = U;
  }
  return bad;
}

}  // namespace

int main() {
  int bad = 0;
  for (int model = 0; model < 4; ++model) bad += check_model(model, 200);
  for (float y : {0.05f, 0.7f, 3.0f, 40.0f}) {
    float g = 0.f;
    const float v = vissm_host_sp_ildj(y, &g);
    const float h = 1e-3f * std::fmax(1.f, y);
    float gp, gm;
    const double num = (vissm_host_sp_ildj(y + h, &gp) - vissm_host_sp_ildj(y - h, &gm)) / (2.0 * h);
    if (!std::isfinite(v) || std::fabs(num - g) > 1e-2 * std::fmax(1.0, std::fabs(num))) {
      std::printf("sp_ildj(%g): %g vs %g\n", y, g, num);
      ++bad;
    }
  }
  float gx = 0.f;
  const float o = vissm_host_obs(1.5f, 1.0f, 1.f, 0.5f, &gx);
  if (!std::isfinite(o) || std::fabs(gx + 2.f) > 1e-5f) { std::printf("obs_term: gx %g\n", gx); ++bad; }
  for (int model = 0; model < 4; ++model) bad += check_sim(model, 50);
  bad += check_sim_dead();
  bad += check_philox();
  bad += check_pf();
  bad += check_ps();
  bad += check_gp();
  bad += check_svf();
  bad += check_mh();
  bad += check_mh_adapt();
  bad += check_svpmmh();
  bad += check_cpm();
  bad += check_colkey();
  bad += check_select();
  for (int which = 0; which < 9; ++which) {
    size_t out[2] = {0, 0};
    vissm_host_abi_layout(which, out);
    if (out[0] == 0 || out[1] >= out[0]) { std::printf("abi layout %d: %zu %zu\n", which, out[0], out[1]); ++bad; }
  }
  std::printf("hostcheck_san: %d failures\n", bad);
  return bad ? 1 : 0;
}
