// libvissm: particle marginal Metropolis-Hastings over theta of the AR, LV and FHN state-space models (vissm_pmmh,
// include/vissm.h; Andrieu, Doucet & Holenstein 2010).  With the fully adapted filter's unbiased estimate of
// p(y | theta) in the acceptance ratio the chain targets p(theta | y) exactly, for any number of particles.
//
// One block per chain, one particle per lane (N = 64 .. 1024 threads); the block walks its iterations in one launch.
// An iteration is
//   the random-walk proposal theta' = theta + L xi and the uniform of the decision (mh_math.hpp), on Philox blocks
//   whose second counter word is 2;
//   the fully adapted filter over the whole series at theta', every particle from x_start: the loop of
//   particle_filter_kernel<MODEL, N, kAdapted> (particle.hip) restated on the same headers (sim_math.hpp,
//   gp_math.hpp, pf_math.hpp) without the cloud, its tile, the traces, ll_inc and ess -- the same rows, normals,
//   weights, integers and four barriers per observed step, so ll' is that entry's loglik for K = C filters at
//   row0 + i C N;
//   the decision in double, and the chain's outputs from lane 0.
// Everything outside the filter is block-uniform: every thread computes the proposal, the prior and the decision from
// the same addresses and the same block sums, so nothing is broadcast and every barrier sits under a block-uniform
// condition.  A filter that dies (W = 0) leaves its loop at once: ll' = -inf whatever follows.
//
// LDS per block = 8 N (C) + 4 S N (gather) + 192 (wave maxima and totals); no tile, so several blocks share a CU up to
// N = 512.  No atomics, no workspace; integer sums and fixed-order doubles: two launches are bitwise equal and chain
// c's bits depend on (seed, row0, C, c, N, it0, the data and its entering state) only.
//
// The stochastic-volatility model has no obs_std / obs_bin observation model and vissm_pmmh refuses it; vissm_sv_pmmh
// (sv_pmmh_kernel, below) runs the same chain around sv_filter.hip's filter of the latent log-volatility.
#include "common.hpp"
#include "gp_math.hpp"
#include "mh_math.hpp"
#include "pf_math.hpp"
#include "pmmh_shell.hpp"  // uni, Out, AdaptOut, load_factor, adapt_step
#include "svf_math.hpp"

namespace vissm {
namespace pmk {

// chol: the fixed variant's prop_chol [P, P], the adaptive variant's chol_in [C, P, P].  adapt_end, target, gamma and a
// are read by the adaptive variant only.
template <int MODEL, int N, bool ADAPT>
__global__ __launch_bounds__(N) void pmmh_kernel(uint64_t seed, uint64_t row0, int C, int n_iter, int it0, int T_total,
                                                 float dt, float obs_std, const float* __restrict__ theta_cur,
                                                 const double* __restrict__ ll_cur, const float* __restrict__ chol,
                                                 const float* __restrict__ prior, const float* __restrict__ x_start,
                                                 const float* __restrict__ obs, const float* __restrict__ obs_bin,
                                                 int adapt_end, double target, double gamma, Out o, AdaptOut a) {
  constexpr int S = VISSM_MODEL_S(MODEL), P = VISSM_MODEL_P(MODEL);
  constexpr int NW = N / 64, LOG2N = pf::log2_of(N);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const size_t c = blockIdx.x;

  __shared__ uint64_t Cs[N];
  __shared__ float xs[S * N];
  __shared__ float wmax[16];
  __shared__ uint64_t wtot[16];
  // the update's doubles, then the factor; the fixed variant never touches it, and it takes no LDS there
  __shared__ double Ws[ADAPT ? adapt_lds_doubles(P) : 1];
  float* const Ls = reinterpret_cast<float*>(Ws + (ADAPT ? mh::adapt_work(P) : 0));

  // the chain's state and the launch's constants: block-uniform
  float th[mh::kMaxP] = {0.f, 0.f, 0.f, 0.f, 0.f};
  float x0[S];
#pragma unroll
  for (int i = 0; i < P; ++i) th[i] = theta_cur[c * P + i];
#pragma unroll
  for (int d = 0; d < S; ++d) x0[d] = x_start[d];
  double ll = ll_cur[c];
  double lp = uni(mh::log_prior(th, prior, P));
  const uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
  if constexpr (ADAPT) load_factor<P>(Ls, chol, c, tid);
  const bool traced = ADAPT && (a.xi_trace || a.alpha_trace || a.eta_trace || a.chol_trace);
  const float R = obs_std * obs_std;

  for (int it = 0; it < n_iter; ++it) {
    const uint64_t frow = mh::row_of(row0, static_cast<uint64_t>(it0) + it, C, c, N);

    // block-uniform: the absolute iteration is below adapt_end
    const bool adapting = ADAPT && static_cast<int64_t>(it0) + it < adapt_end;
    // The factor and the prior are read again in every iteration (scalar loads): held over the filter loop, their
    // twenty-five doubles would take fifty vector registers, and the 1024-lane FHN block would spill.  The adaptive
    // variant's factor is the chain's own, in LDS: every thread reads the same words.
    const float *Lc = ADAPT ? Ls : chol, *pr = prior;
    if constexpr (ADAPT)
      asm volatile("" : "+s"(pr));
    else
      asm volatile("" : "+s"(Lc), "+s"(pr));

    // the proposal
    float thp[mh::kMaxP] = {0.f, 0.f, 0.f, 0.f, 0.f};
    {
      float xi[8], v[4];
      box_muller4(mh::words(0u, frow, seed), v);
#pragma unroll
      for (int i = 0; i < 4; ++i) xi[i] = v[i];
      box_muller4(mh::words(1u, frow, seed), v);
#pragma unroll
      for (int i = 0; i < 4; ++i) xi[4 + i] = v[i];
      mh::propose(th, Lc, xi, P, thp);
#pragma unroll
      for (int i = 0; i < P; ++i) thp[i] = uni(thp[i]);
    }
    // every wave has read the factor before thread 0 rewrites it (the filter loop below may pass no barrier)
    if (adapting) __syncthreads();

    // the fully adapted filter at theta' over steps 0 .. T_total - 1
    const sim::Par par = sim::prepare<MODEL>(thp, dt);
    float x[sim::kMaxS] = {0.f, 0.f};
#pragma unroll
    for (int d = 0; d < S; ++d) x[d] = x0[d];
    sim::start<MODEL>(x);
    double llp = 0.0;
    const uint64_t row = frow + static_cast<uint64_t>(tid);
    uint32_t j = 0u, g = 0u;  // stream entry of the step's first normal and its Philox group
    float cur[4], nxt[4];
    draw4(g, row, k0, k1, cur);
    draw4(g + 1, row, k0, k1, nxt);

    for (int ta = 0; ta < T_total; ++ta) {
      const uint32_t qd = j & 3u;
      float n[2];
      if constexpr (S == 2) {
        n[0] = qd ? cur[2] : cur[0];
        n[1] = qd ? cur[3] : cur[1];
      } else {
        n[0] = qd == 0 ? cur[0] : qd == 1 ? cur[1] : qd == 2 ? cur[2] : cur[3];
        n[1] = 0.f;
      }
      // every thread reads the same addresses: block-uniform
      float yv[S], bv[S];
      bool observed = false;
#pragma unroll
      for (int d = 0; d < S; ++d) {
        bv[d] = obs_bin[static_cast<size_t>(d) * T_total + ta];
        yv[d] = obs[static_cast<size_t>(d) * T_total + ta];
        observed = observed || bv[d] != 0.f;
      }
      if (!observed) {
        sim::advance<MODEL>(x, par, n, 0.f, nullptr);
      } else {
        const bool ok = sim::alive(MODEL, x);
        const float lw = ok ? gp::state_logw<MODEL>(x, par, yv, bv, R) : -INFINITY;
        const float wm = wave_max(lw);
        if (lane == 0) wmax[wid] = wm;
#pragma unroll
        for (int d = 0; d < S; ++d) xs[d * N + tid] = x[d];
        __syncthreads();  // A
        float m = wmax[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) m = fmaxf(m, wmax[w]);
        m = uni(m);  // the same LDS words in every thread
        const uint64_t q = pf::quantise(lw, m, ok);
        const uint64_t cs = wave_scan(q, lane);
        if (lane == 63) wtot[wid] = cs;
        __syncthreads();  // B
        uint64_t before = 0, W = 0;
#pragma unroll 2
        for (int w = 0; w < NW; ++w) {
          if (w < wid) before += wtot[w];
          W += wtot[w];
        }
        Cs[tid] = cs + before;
        W = uni(W);  // block-uniform: the branches below are scalar
        __syncthreads();  // C
        if (W > 0) {
          const uint32_t U = pf::resample_u(seed, static_cast<uint32_t>(ta), frow);
          int anc = pf::ancestor(Cs, N, pf::threshold(static_cast<uint32_t>(tid), U, W, LOG2N));
          anc = min(anc, N - 1);  // tau < W = C[N - 1]: never taken
#pragma unroll
          for (int d = 0; d < S; ++d) x[d] = xs[d * N + anc];
          gp::advance<MODEL>(x, par, yv, bv, R, n);
          llp = uni(llp + pf::ll_increment(m, W, N));
        } else {  // no live particle with a weight: the proposal is dead
          llp = -INFINITY;
        }
        __syncthreads();  // D: the gather is over before the next observed step overwrites the staging arrays
        if (W == 0) break;
      }
      j += S;
      if ((j & 3u) == 0u) {  // uniform: the next step opens a new group; draw the one after it now
#pragma unroll
        for (int i = 0; i < 4; ++i) cur[i] = nxt[i];
        ++g;
        draw4(g + 1, row, k0, k1, nxt);
      }
    }

    // the decision (its uniform and the proposal's prior are not needed before: they are not kept over the filter)
    const double lpp = mh::log_prior(thp, pr, P);
    const double logu = mh::log_uniform(mh::words(2u, frow, seed).x);
    // the acceptance probability, from the state before the decision
    double al = 0.0;
    if (adapting || traced) al = uni(mh::accept_prob(llp, ll, lpp, lp));
    const bool acc =__builtin_amdgcn_readfirstlane(mh::accept(logu, llp, ll, lpp, lp) ? 1 : 0) != 0;
    if (acc) {
#pragma unroll
      for (int i = 0; i < P; ++i) th[i] = thp[i];
      ll = uni(llp);
      lp = uni(lpp);
    }
    if (tid == 0) {
      const size_t e = c * static_cast<size_t>(n_iter) + it;
#pragma unroll
      for (int i = 0; i < P; ++i) o.theta_chain[e * P + i] = th[i];
      o.ll_chain[e] = ll;
      o.accept[e] = acc ? 1 : 0;
      if (o.theta_prop) {
#pragma unroll
        for (int i = 0; i < P; ++i) o.theta_prop[e * P + i] = thp[i];
      }
      if (o.ll_prop) o.ll_prop[e] = llp;
      if (o.logu) o.logu[e] = logu;
      // the update, in a scope of its own: nothing of it is live over the filter loop
      if (adapting || traced)
        adapt_step<P>(Ls, Ws, frow, seed, adapting, static_cast<int64_t>(it0) + it, al, target, gamma, a, e);
    }
    // thread 0's factor is in LDS before the next iteration's proposal reads it
    if (adapting) __syncthreads();
  }
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < P; ++i) o.theta_end[c * P + i] = th[i];
    o.ll_end[c] = ll;
    if constexpr (ADAPT) {
#pragma unroll
      for (int i = 0; i < P * P; ++i) a.chol_end[c * (P * P) + i] = Ls[i];
    }
  }
}

// ---- stochastic volatility ----------------------------------------------------------------------------------------
// The same iteration shell around sv_filter_kernel's loop (sv_filter.hip) with t0 = 0 and H = T_total: the particle is
// the latent h alone, the observed series y [T_total + 1] the state's first coordinate.  Every step is observed: step
// ta scores the pre-step h on (y[ta], y[ta + 1]), resamples and moves the ancestor's h with the lane's own normal
// (AR's one-normal stream), so ll' is vissm_sv_filter's loglik for K = C filters at row0 + i C N from h_start.  The
// shell is restated here, not shared with pmmh_kernel as a device function: that costs 5 % here.
// LDS per block = 8 N (C) + 4 N (gather) + 192.
constexpr int kSvP = VISSM_MODEL_P(VISSM_MODEL_SV);

template <int N, bool ADAPT>
__global__ __launch_bounds__(N) void sv_pmmh_kernel(uint64_t seed, uint64_t row0, int C, int n_iter, int it0,
                                                    int T_total, float dt, const float* __restrict__ theta_cur,
                                                    const double* __restrict__ ll_cur, const float* __restrict__ chol,
                                                    const float* __restrict__ prior, const float* __restrict__ h_start,
                                                    const float* __restrict__ obs, int adapt_end, double target,
                                                    double gamma, Out o, AdaptOut a) {
  constexpr int P = kSvP;
  constexpr int NW = N / 64, LOG2N = pf::log2_of(N);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const size_t c = blockIdx.x;

  __shared__ uint64_t Cs[N];
  __shared__ float xs[N];
  __shared__ float wmax[16];
  __shared__ uint64_t wtot[16];
  // the update's doubles, then the factor; the fixed variant never touches it, and it takes no LDS there
  __shared__ double Ws[ADAPT ? adapt_lds_doubles(P) : 1];
  float* const Ls = reinterpret_cast<float*>(Ws + (ADAPT ? mh::adapt_work(P) : 0));

  // the chain's state and the launch's constants: block-uniform
  float th[mh::kMaxP] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < P; ++i) th[i] = theta_cur[c * P + i];
  float h0 = h_start[0];
  if (!__builtin_isfinite(h0)) h0 = sim::quiet_nan();
  double ll = ll_cur[c];
  double lp = uni(mh::log_prior(th, prior, P));
  const uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
  if constexpr (ADAPT) load_factor<P>(Ls, chol, c, tid);
  const bool traced = ADAPT && (a.xi_trace || a.alpha_trace || a.eta_trace || a.chol_trace);

  for (int it = 0; it < n_iter; ++it) {
    const uint64_t frow = mh::row_of(row0, static_cast<uint64_t>(it0) + it, C, c, N);

    // block-uniform: the absolute iteration is below adapt_end
    const bool adapting = ADAPT && static_cast<int64_t>(it0) + it < adapt_end;
    // the factor (or the chain's own, in LDS) and the prior are read again in every iteration, as in pmmh_kernel
    const float *Lc = ADAPT ? Ls : chol, *pr = prior;
    if constexpr (ADAPT)
      asm volatile("" : "+s"(pr));
    else
      asm volatile("" : "+s"(Lc), "+s"(pr));

    // the proposal
    float thp[mh::kMaxP] = {0.f, 0.f, 0.f, 0.f, 0.f};
    {
      float xi[8], v[4];
      box_muller4(mh::words(0u, frow, seed), v);
#pragma unroll
      for (int i = 0; i < 4; ++i) xi[i] = v[i];
      box_muller4(mh::words(1u, frow, seed), v);
#pragma unroll
      for (int i = 0; i < 4; ++i) xi[4 + i] = v[i];
      mh::propose(th, Lc, xi, P, thp);
#pragma unroll
      for (int i = 0; i < P; ++i) thp[i] = uni(thp[i]);
    }
    // every wave has read the factor before thread 0 rewrites it (the filter loop below may pass no barrier)
    if (adapting) __syncthreads();

    // the filter at theta' over steps 0 .. T_total - 1
    const sim::Par par = sim::prepare<VISSM_MODEL_SV>(thp, dt);
    float h = h0;
    double llp = 0.0;
    const uint64_t row = frow + static_cast<uint64_t>(tid);
    uint32_t j = 0u, g = 0u;  // stream entry of the step's normal and its Philox group
    float cur[4], nxt[4];
    draw4(g, row, k0, k1, cur);
    draw4(g + 1, row, k0, k1, nxt);

    for (int ta = 0; ta < T_total; ++ta) {
      const uint32_t qd = j & 3u;
      const float n = qd == 0 ? cur[0] : qd == 1 ? cur[1] : qd == 2 ? cur[2] : cur[3];
      // every thread reads the same addresses: block-uniform
      const svf::Obs ob = svf::obs_prep(obs[ta], obs[static_cast<size_t>(ta) + 1], par);
      const bool ok = __builtin_isfinite(h);
      const float lw = svf::state_logw(h, ob);
      const float wm = wave_max(lw);
      if (lane == 0) wmax[wid] = wm;
      xs[tid] = h;
      __syncthreads();  // A
      float m = wmax[0];
#pragma unroll
      for (int w = 1; w < NW; ++w) m = fmaxf(m, wmax[w]);
      m = uni(m);  // the same LDS words in every thread
      const uint64_t q = pf::quantise(lw, m, ok);
      const uint64_t cs = wave_scan(q, lane);
      if (lane == 63) wtot[wid] = cs;
      __syncthreads();  // B
      uint64_t before = 0, W = 0;
#pragma unroll 2
      for (int w = 0; w < NW; ++w) {
        if (w < wid) before += wtot[w];
        W += wtot[w];
      }
      Cs[tid] = cs + before;
      W = uni(W);  // block-uniform: the branches below are scalar
      __syncthreads();  // C
      if (W > 0) {
        const uint32_t U = pf::resample_u(seed, static_cast<uint32_t>(ta), frow);
        int anc = pf::ancestor(Cs, N, pf::threshold(static_cast<uint32_t>(tid), U, W, LOG2N));
        anc = min(anc, N - 1);  // tau < W = C[N - 1]: never taken
        h = svf::move(xs[anc], par, n);
        llp = uni(llp + pf::ll_increment(m, W, N));
      } else {  // no live particle with a weight (a zero in y gives NaN weights): the proposal is dead
        llp = -INFINITY;
      }
      __syncthreads();  // D: the gather is over before the next step overwrites the staging arrays
      if (W == 0) break;
      ++j;
      if ((j & 3u) == 0u) {  // uniform: the next step opens a new group; draw the one after it now
#pragma unroll
        for (int i = 0; i < 4; ++i) cur[i] = nxt[i];
        ++g;
        draw4(g + 1, row, k0, k1, nxt);
      }
    }

    // the decision
    const double lpp = mh::log_prior(thp, pr, P);
    const double logu = mh::log_uniform(mh::words(2u, frow, seed).x);
    // the acceptance probability, from the state before the decision
    double al = 0.0;
    if (adapting || traced) al = uni(mh::accept_prob(llp, ll, lpp, lp));
    const bool acc =__builtin_amdgcn_readfirstlane(mh::accept(logu, llp, ll, lpp, lp) ? 1 : 0) != 0;
    if (acc) {
#pragma unroll
      for (int i = 0; i < P; ++i) th[i] = thp[i];
      ll = uni(llp);
      lp = uni(lpp);
    }
    if (tid == 0) {
      const size_t e = c * static_cast<size_t>(n_iter) + it;
#pragma unroll
      for (int i = 0; i < P; ++i) o.theta_chain[e * P + i] = th[i];
      o.ll_chain[e] = ll;
      o.accept[e] = acc ? 1 : 0;
      if (o.theta_prop) {
#pragma unroll
        for (int i = 0; i < P; ++i) o.theta_prop[e * P + i] = thp[i];
      }
      if (o.ll_prop) o.ll_prop[e] = llp;
      if (o.logu) o.logu[e] = logu;
      // the update, in a scope of its own: nothing of it is live over the filter loop
      if (adapting || traced)
        adapt_step<P>(Ls, Ws, frow, seed, adapting, static_cast<int64_t>(it0) + it, al, target, gamma, a, e);
    }
    // thread 0's factor is in LDS before the next iteration's proposal reads it
    if (adapting) __syncthreads();
  }
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < P; ++i) o.theta_end[c * P + i] = th[i];
    o.ll_end[c] = ll;
    if constexpr (ADAPT) {
#pragma unroll
      for (int i = 0; i < P * P; ++i) a.chol_end[c * (P * P) + i] = Ls[i];
    }
  }
}

// the checks the two entries share, with the entry's name in the message
int check_chain_args(const char* name, const VissmPmmhDesc* d, bool pointers, bool pointers_iter, bool pointers_t) {
  VISSM_CHECK_ARG(pf::valid_n(d->N), "%s: N=%d particles (64, 128, 256, 512 or 1024)", name, d->N);
  VISSM_CHECK_ARG(d->C >= 1, "%s: C=%d chains (at least one)", name, d->C);
  VISSM_CHECK_ARG(d->n_iter >= 0 && d->it0 >= 0 && static_cast<int64_t>(d->it0) + d->n_iter < (int64_t{1} << 31),
                  "%s: bad iterations it0=%d n_iter=%d", name, d->it0, d->n_iter);
  VISSM_CHECK_ARG(pointers, "%s: null pointer", name);
  VISSM_CHECK_ARG(d->n_iter == 0 || pointers_iter, "%s: null pointer (n_iter > 0)", name);
  VISSM_CHECK_ARG(d->T_total <= 0 || pointers_t, "%s: null pointer (T_total > 0)", name);
  return VISSM_OK;
}

// the checks the two adaptive entries add
int check_adapt_args(const char* name, int32_t adapt_end, double target_accept, double gamma, const void* chol_in,
                     const void* chol_end) {
  VISSM_CHECK_ARG(adapt_end >= 0, "%s: adapt_end=%d (an absolute iteration, at least 0)", name, adapt_end);
  // (a NaN fails either comparison)
  VISSM_CHECK_ARG(target_accept > 0.0 && target_accept < 1.0, "%s: target_accept=%g outside (0, 1)", name,
                  target_accept);
  VISSM_CHECK_ARG(gamma > 0.0 && gamma <= 1.0, "%s: gamma=%g outside (0, 1]", name, gamma);
  VISSM_CHECK_ARG(chol_in && chol_end, "%s: null pointer (chol_in, chol_end)", name);
  return VISSM_OK;
}

// What the fixed entry and its adaptive twin do, under the entry's name: the checks (host arithmetic only, before any
// GPU call) and the launch.  chol is prop_chol or chol_in; the fixed entries pass ADAPT = false, an empty AdaptOut and
// adaptive scalars that nothing reads.
template <bool ADAPT>
int run_pmmh(const char* name, const VissmPmmhDesc* d, uint64_t seed, uint64_t row0, const float* theta_cur,
             const double* ll_cur, const float* chol, const float* prior, const float* x_start, const float* obs,
             const float* obs_bin, int32_t adapt_end, double target_accept, double gamma, const Out& o,
             const AdaptOut& a, void* stream) {
  VISSM_CHECK_ARG(d, "%s: null descriptor", name);
  VISSM_CHECK_ARG(d->model != VISSM_MODEL_SV,
                  "%s: no observation model for SV (its first coordinate is the observed series)", name);
  VISSM_CHECK_ARG(d->model == VISSM_MODEL_AR || d->model == VISSM_MODEL_LV || d->model == VISSM_MODEL_FHN,
                  "%s: unknown model %d", name, d->model);
  if (const int rc = check_chain_args(
          name, d, theta_cur && ll_cur && (ADAPT || chol) && prior && x_start && o.theta_end && o.ll_end,
          o.theta_chain && o.ll_chain && o.accept, obs && obs_bin))
    return rc;
  if constexpr (ADAPT)
    if (const int rc = check_adapt_args(name, adapt_end, target_accept, gamma, chol, a.chol_end)) return rc;
  VISSM_CHECK_ARG(d->T_total >= 0, "%s: T_total=%d", name, d->T_total);
  const int S = VISSM_MODEL_S(d->model);
  VISSM_CHECK_ARG(static_cast<int64_t>(d->T_total) * S < (int64_t{1} << 31), "%s: T_total S = %d %d reaches 2^31", name,
                  d->T_total, S);
  // (a NaN fails the first comparison, an infinity the second)
  VISSM_CHECK_ARG(d->obs_std > 0.f && d->obs_std <= 3.4028234e38f, "%s: a positive, finite obs_std expected, got %g",
                  name, static_cast<double>(d->obs_std));
  dispatch_model(d->model, [&](auto model) {
    dispatch_n(d->N, [&](auto n) {
      hipLaunchKernelGGL((pmmh_kernel<decltype(model)::value, decltype(n)::value, ADAPT>), dim3(d->C), dim3(d->N), 0,
                         as_stream(stream), seed, row0, d->C, d->n_iter, d->it0, d->T_total, d->dt, d->obs_std,
                         theta_cur, ll_cur, chol, prior, x_start, obs, obs_bin, adapt_end, target_accept, gamma, o, a);
    });
  });
  VISSM_CHECK_LAUNCH(name);
  return VISSM_OK;
}

// the same for the stochastic-volatility pair; name is "sv_" and the name of the entry that has the other models
template <bool ADAPT>
int run_sv_pmmh(const char* name, const VissmPmmhDesc* d, uint64_t seed, uint64_t row0, const float* theta_cur,
                const double* ll_cur, const float* chol, const float* prior, const float* h_start, const float* obs,
                int32_t adapt_end, double target_accept, double gamma, const Out& o, const AdaptOut& a, void* stream) {
  VISSM_CHECK_ARG(d, "%s: null descriptor", name);
  VISSM_CHECK_ARG(d->model == VISSM_MODEL_SV, "%s: model %d is not SV (vissm_%s has the others)", name, d->model,
                  name + 3);
  if (const int rc = check_chain_args(
          name, d, theta_cur && ll_cur && (ADAPT || chol) && prior && h_start && o.theta_end && o.ll_end,
          o.theta_chain && o.ll_chain && o.accept, obs != nullptr))
    return rc;
  if constexpr (ADAPT)
    if (const int rc = check_adapt_args(name, adapt_end, target_accept, gamma, chol, a.chol_end)) return rc;
  // (the series holds T_total + 1 values and step ta reads y[ta + 1])
  VISSM_CHECK_ARG(d->T_total >= 0 && d->T_total < 2147483647, "%s: T_total=%d", name, d->T_total);
  // (a NaN fails the first comparison, an infinity the second)
  VISSM_CHECK_ARG(d->dt > 0.f && d->dt <= 3.4028234e38f, "%s: dt must be positive and finite, got %g", name,
                  static_cast<double>(d->dt));
  dispatch_n(d->N, [&](auto n) {
    hipLaunchKernelGGL((sv_pmmh_kernel<decltype(n)::value, ADAPT>), dim3(d->C), dim3(d->N), 0, as_stream(stream), seed,
                       row0, d->C, d->n_iter, d->it0, d->T_total, d->dt, theta_cur, ll_cur, chol, prior, h_start, obs,
                       adapt_end, target_accept, gamma, o, a);
  });
  VISSM_CHECK_LAUNCH(name);
  return VISSM_OK;
}

}  // namespace pmk
}  // namespace vissm

using namespace vissm;
using namespace vissm::pmk;

extern "C" int32_t vissm_pmmh_lds_bytes(int32_t model, int32_t N) {
  if (!(model == VISSM_MODEL_AR || model == VISSM_MODEL_LV || model == VISSM_MODEL_FHN) || !pf::valid_n(N)) return 0;
  return 8 * N + 4 * VISSM_MODEL_S(model) * N + 16 * (4 + 8);
}

extern "C" int vissm_pmmh(const VissmPmmhDesc* d, uint64_t seed, uint64_t row0, const float* theta_cur,
                          const double* ll_cur, const float* prop_chol, const float* prior, const float* x_start,
                          const float* obs, const float* obs_bin, float* theta_chain, double* ll_chain,
                          int32_t* accept, float* theta_end, double* ll_end, float* theta_prop, double* ll_prop,
                          double* logu, void* stream) {
  return run_pmmh<false>("pmmh", d, seed, row0, theta_cur, ll_cur, prop_chol, prior, x_start, obs, obs_bin, 0, 0.0, 0.0,
                         Out{theta_chain, ll_chain, accept, theta_end, ll_end, theta_prop, ll_prop, logu}, AdaptOut{},
                         stream);
}

extern "C" int32_t vissm_sv_pmmh_lds_bytes(int32_t N) {
  if (!pf::valid_n(N)) return 0;
  return 8 * N + 4 * N + 16 * (4 + 8);
}

extern "C" int vissm_sv_pmmh(const VissmPmmhDesc* d, uint64_t seed, uint64_t row0, const float* theta_cur,
                             const double* ll_cur, const float* prop_chol, const float* prior, const float* h_start,
                             const float* obs, float* theta_chain, double* ll_chain, int32_t* accept, float* theta_end,
                             double* ll_end, float* theta_prop, double* ll_prop, double* logu, void* stream) {
  return run_sv_pmmh<false>("sv_pmmh", d, seed, row0, theta_cur, ll_cur, prop_chol, prior, h_start, obs, 0, 0.0, 0.0,
                            Out{theta_chain, ll_chain, accept, theta_end, ll_end, theta_prop, ll_prop, logu},
                            AdaptOut{}, stream);
}

// the twin's + 8 (P P + 2 P) (the update's doubles) + 8 ceil(P P / 2) (the chain's factor)
extern "C" int32_t vissm_pmmh_adaptive_lds_bytes(int32_t model, int32_t N) {
  const int32_t twin = vissm_pmmh_lds_bytes(model, N);
  const int P = twin ? VISSM_MODEL_P(model) : 0;
  return twin ? twin + 8 * adapt_lds_doubles(P) : 0;
}

extern "C" int vissm_pmmh_adaptive(const VissmPmmhDesc* d, uint64_t seed, uint64_t row0, const float* theta_cur,
                                   const double* ll_cur, const float* chol_in, const float* prior,
                                   const float* x_start, const float* obs, const float* obs_bin, int32_t adapt_end,
                                   double target_accept, double gamma, float* theta_chain, double* ll_chain,
                                   int32_t* accept, float* theta_end, double* ll_end, float* chol_end,
                                   float* theta_prop, double* ll_prop, double* logu, float* xi_trace,
                                   double* alpha_trace, double* eta_trace, float* chol_trace, void* stream) {
  return run_pmmh<true>("pmmh_adaptive", d, seed, row0, theta_cur, ll_cur, chol_in, prior, x_start, obs, obs_bin,
                        adapt_end, target_accept, gamma,
                        Out{theta_chain, ll_chain, accept, theta_end, ll_end, theta_prop, ll_prop, logu},
                        AdaptOut{chol_end, xi_trace, alpha_trace, eta_trace, chol_trace}, stream);
}

// the twin's + 8 (P P + 2 P) + 8 ceil(P P / 2), P = 4
extern "C" int32_t vissm_sv_pmmh_adaptive_lds_bytes(int32_t N) {
  const int32_t twin = vissm_sv_pmmh_lds_bytes(N);
  return twin ? twin + 8 * adapt_lds_doubles(kSvP) : 0;
}

extern "C" int vissm_sv_pmmh_adaptive(const VissmPmmhDesc* d, uint64_t seed, uint64_t row0, const float* theta_cur,
                                      const double* ll_cur, const float* chol_in, const float* prior,
                                      const float* h_start, const float* obs, int32_t adapt_end, double target_accept,
                                      double gamma, float* theta_chain, double* ll_chain, int32_t* accept,
                                      float* theta_end, double* ll_end, float* chol_end, float* theta_prop,
                                      double* ll_prop, double* logu, float* xi_trace, double* alpha_trace,
                                      double* eta_trace, float* chol_trace, void* stream) {
  return run_sv_pmmh<true>("sv_pmmh_adaptive", d, seed, row0, theta_cur, ll_cur, chol_in, prior, h_start, obs,
                           adapt_end, target_accept, gamma,
                           Out{theta_chain, ll_chain, accept, theta_end, ll_end, theta_prop, ll_prop, logu},
                           AdaptOut{chol_end, xi_trace, alpha_trace, eta_trace, chol_trace}, stream);
}

