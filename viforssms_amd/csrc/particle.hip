// libvissm: bootstrap particle filter of the AR, LV and FHN state-space models (vissm_particle_filter,
// include/vissm.h) -- an estimate of log p(y | theta) and the filtering cloud that does not come out of the flows.
// The reference has no filter: its terms restate the reference's transition and observation models (AR.py:168-176,
// lotka_volterra_partial.py:234-261, fitz_nag_NVP.py:232-255) as a propagate / weight / resample loop.
//
// One block per filter, one particle per lane (N = 64 .. 1024 threads).  A step is sim::advance (sim_math.hpp, the
// forecast's Euler-Maruyama step with its death rule) on the normals vissm_sde_simulate gives the same Philox row,
// drawn one group ahead of the chain; at an observed step the block then weights (em::obs_term), reduces, scans and
// resamples in integers (pf_math.hpp):
//   barrier A  wave maxima of logw and the states (for the gather) are in LDS
//   barrier B  wave totals of q (inclusive uint64 wave scan) and of q^2 (double) are in LDS
//   barrier C  the cumulative sum C is in LDS; each lane binary-searches it for its threshold and gathers its ancestor
//   barrier D  the gather is over before the next observed step overwrites the staging arrays
// "Observed" is read by every thread from the same addresses (obs_bin[:, t0 + t]), so it is block-uniform and every
// barrier sits under a block-uniform condition; a dead filter keeps walking the loop and its barriers.  Unobserved
// steps have no barrier.  Sums are integers or fixed-order doubles (wave butterfly, then the waves in order):
// two launches are bitwise equal and filter k's bits depend on (seed, row0 + k N, theta_k, N, data) only.
//
// Output cloud is sample-major [K N][S][H].  A lane that stored its own row would write one cache line per lane, so
// the block stages DEPTH steps of its N particles in LDS -- plane d, particle i, step t at i DEPTH + (t ^ (i mod
// DEPTH)), the swizzle of simulate.hip's tile -- and writes them out as row segments of DEPTH consecutive steps.
// DEPTH = min(64, 128 KiB / (4 S N)): 64 steps (256-byte segments) up to N = 512 for AR and N = 256 for LV / FHN,
// 32 steps (128 bytes) at AR N = 1024 and LV / FHN N = 512, and 16 steps (64 bytes) at LV / FHN N = 1024, where 32
// steps of 2048 values would need 256 KiB, more than the CU's LDS.  LDS per block = 4 S N DEPTH (tile) + 8 N (C)
// + 4 S N (gather) + 8 DEPTH (ll_inc, ess) + 320 (wave partials): at most 147,904 bytes (LV / FHN, N = 1024) of
// the 160 KiB a block may declare (vissm_particle_filter_lds_bytes).
//
// The fully adapted filter (vissm_particle_filter_adapted; gp_math.hpp) is the same body with PROPOSAL = kAdapted:
// geometry, stream, tile, integer pipeline, outputs and chaining are the bootstrap's, and an unobserved step is
// sim::advance, bitwise.  At an observed step each lane scores its *pre-step* state on the predictive p(y_t | x_t-1)
// (gp::state_logw), the block resamples behind the same four barriers, and slot j gathers ancestor a_j's pre-step
// state (S words; mu and Sigma are recomputed rather than staged, five more words per particle that the LV / FHN
// N = 1024 block's LDS does not have) and draws x' from p(x_t | x_t-1, y_t) of that state with its own normals
// (gp::advance, with the death rule).  The cloud then holds the post-propagation particles, an equally weighted
// sample of p(x_t | y_1:t); an LV draw may leave the orthant after the resampling, so unlike the bootstrap's cloud
// it may hold NaN particles at observed steps.  They get q = 0 at the next observed step.
#include "common.hpp"
#include "gp_math.hpp"
#include "pf_math.hpp"

namespace vissm {
namespace pfk {

constexpr int kTileBytes = 128 * 1024;
constexpr int kBootstrap = 0, kAdapted = 1;  // PROPOSAL

constexpr int tile_depth(int S, int N) {
  const int d = kTileBytes / (4 * S * N);
  return d > 64 ? 64 : d;
}

template <int MODEL, int N, int PROPOSAL>
__global__ __launch_bounds__(N) void particle_filter_kernel(
    uint64_t seed, uint64_t row0, int H, int t0, int T_total, float dt, float obs_std, const float* __restrict__ theta,
    const float* __restrict__ x_start, const float* __restrict__ obs, const float* __restrict__ obs_bin,
    const double* __restrict__ loglik_in, double* __restrict__ loglik, float* __restrict__ ll_inc,
    float* __restrict__ ess_out, float* __restrict__ state_end, float* __restrict__ cloud,
    unsigned long long* __restrict__ q_trace, int32_t* __restrict__ anc_trace) {
  constexpr int S = VISSM_MODEL_S(MODEL), P = VISSM_MODEL_P(MODEL);
  constexpr int NW = N / 64, LOG2N = pf::log2_of(N);
  constexpr int DEPTH = tile_depth(S, N);
  static_assert(DEPTH >= 16 && (DEPTH & (DEPTH - 1)) == 0 && N % DEPTH == 0, "tile depth");
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const size_t k = blockIdx.x;
  const size_t p = k * N + tid;  // the particle's row in the [K N] arrays

  __shared__ float tile[S * N * DEPTH];
  __shared__ uint64_t Cs[N];
  __shared__ float xs[S * N];
  __shared__ float ll_tile[DEPTH], ess_tile[DEPTH];
  __shared__ float wmax[16];
  __shared__ uint64_t wtot[16];
  __shared__ double wsq[16];

  float th[sim::kMaxP] = {0.f, 0.f, 0.f, 0.f, 0.f};
  float x[sim::kMaxS] = {0.f, 0.f};
#pragma unroll
  for (int i = 0; i < P; ++i) th[i] = theta[k * P + i];
#pragma unroll
  for (int d = 0; d < S; ++d) x[d] = x_start[p * S + d];
  const sim::Par par = sim::prepare<MODEL>(th, dt);
  sim::start<MODEL>(x);

  // block-uniform: a filter that died in an earlier call stays dead
  double ll = loglik_in ? loglik_in[k] : 0.0;
  bool dead = ll == -INFINITY;
  if (dead) {
#pragma unroll
    for (int d = 0; d < S; ++d) x[d] = sim::quiet_nan();
  }

  const uint64_t frow = row0 + k * N;  // the filter's first Philox row: keys its resampling integers
  const uint64_t row = frow + static_cast<uint64_t>(tid);
  const uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
  uint32_t j = static_cast<uint32_t>(t0) * S;  // stream entry of the step's first normal ((t0 + H) S < 2^31)
  uint32_t g = j >> 2;                         // its Philox group; S divides 4, so a step never straddles two
  float cur[4], nxt[4];
  draw4(g, row, k0, k1, cur);
  draw4(g + 1, row, k0, k1, nxt);

  for (int tb = 0; tb < H; tb += DEPTH) {
    const int nt = min(DEPTH, H - tb);
    for (int tt = 0; tt < nt; ++tt) {
      const int ta = t0 + tb + tt;  // absolute step
      const uint32_t qd = j & 3u;
      float n[2];
      if constexpr (S == 2) {
        n[0] = qd ? cur[2] : cur[0];
        n[1] = qd ? cur[3] : cur[1];
      } else {
        n[0] = qd == 0 ? cur[0] : qd == 1 ? cur[1] : qd == 2 ? cur[2] : cur[3];
        n[1] = 0.f;
      }
      if constexpr (PROPOSAL == kBootstrap) sim::advance<MODEL>(x, par, n, 0.f, nullptr);

      // every thread reads the same addresses: block-uniform
      float yv[S], bv[S];
      bool observed = false;
#pragma unroll
      for (int d = 0; d < S; ++d) {
        bv[d] = obs_bin[static_cast<size_t>(d) * T_total + ta];
        yv[d] = obs[static_cast<size_t>(d) * T_total + ta];
        observed = observed || bv[d] != 0.f;
      }
      if constexpr (PROPOSAL == kAdapted) {  // an observed step moves after the resampling
        if (!observed) sim::advance<MODEL>(x, par, n, 0.f, nullptr);
      }

      float inc = dead ? sim::quiet_nan() : 0.f, es = dead ? sim::quiet_nan() : static_cast<float>(N);
      uint64_t q = 0;
      int anc = tid;
      if (observed) {
        const bool ok = sim::alive(MODEL, x);
        float lw;
        if constexpr (PROPOSAL == kBootstrap) lw = ok ? pf::obs_logw(S, x, yv, bv, obs_std) : -INFINITY;
        else lw = ok ? gp::state_logw<MODEL>(x, par, yv, bv, obs_std * obs_std) : -INFINITY;
        const float wm = wave_max(lw);
        if (lane == 0) wmax[wid] = wm;
#pragma unroll
        for (int d = 0; d < S; ++d) xs[d * N + tid] = x[d];
        __syncthreads();  // A
        float m = wmax[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) m = fmaxf(m, wmax[w]);
        q = pf::quantise(lw, m, ok);
        const uint64_t c = wave_scan(q, lane);
        const double qq = static_cast<double>(q);
        const double s2 = wave_sum(qq * qq);
        if (lane == 63) wtot[wid] = c;
        if (lane == 0) wsq[wid] = s2;
        __syncthreads();  // B
        uint64_t before = 0, W = 0;
        double Q2 = 0.0;
#pragma unroll 2  // (all sixteen partials in flight at once cost the 1024-lane block registers it does not have)
        for (int w = 0; w < NW; ++w) {
          if (w < wid) before += wtot[w];
          W += wtot[w];
          Q2 += wsq[w];
        }
        Cs[tid] = c + before;
        __syncthreads();  // C
        if (W > 0) {
          const uint32_t U = pf::resample_u(seed, static_cast<uint32_t>(ta), frow);
          anc = pf::ancestor(Cs, N, pf::threshold(static_cast<uint32_t>(tid), U, W, LOG2N));
          anc = min(anc, N - 1);  // tau < W = C[N - 1]: never taken
#pragma unroll
          for (int d = 0; d < S; ++d) x[d] = xs[d * N + anc];
          if constexpr (PROPOSAL == kAdapted) gp::advance<MODEL>(x, par, yv, bv, obs_std * obs_std, n);
          const double li = pf::ll_increment(m, W, N);
          ll += li;
          inc = static_cast<float>(li);
          es = static_cast<float>(pf::ess(W, Q2));
        } else {  // no live particle with a weight: the filter is dead from here on
          dead = true;
          ll = -INFINITY;
          inc = es = sim::quiet_nan();
#pragma unroll
          for (int d = 0; d < S; ++d) x[d] = sim::quiet_nan();
        }
        __syncthreads();  // D
      }
      if (q_trace) q_trace[(k * H + tb + tt) * N + tid] = q;
      if (anc_trace) anc_trace[(k * H + tb + tt) * N + tid] = anc;
      if (tid == 0) {
        ll_tile[tt] = inc;
        ess_tile[tt] = es;
      }
      if (cloud) {
        const int at = tid * DEPTH + (tt ^ (tid & (DEPTH - 1)));
#pragma unroll
        for (int d = 0; d < S; ++d) tile[d * N * DEPTH + at] = x[d];
      }
      j += S;
      if ((j & 3u) == 0u) {  // uniform: the next step opens a new group; draw the one after it now
#pragma unroll
        for (int i = 0; i < 4; ++i) cur[i] = nxt[i];
        ++g;
        draw4(g + 1, row, k0, k1, nxt);
      }
    }
    __syncthreads();
    if (tid < nt) {
      ll_inc[k * H + tb + tid] = ll_tile[tid];
      ess_out[k * H + tb + tid] = ess_tile[tid];
    }
    if (cloud) {
      // pass r: N / DEPTH rows at once, DEPTH consecutive lanes on the consecutive steps of one row
      const int ts = tid & (DEPTH - 1), sub = tid / DEPTH;
#pragma unroll
      for (int d = 0; d < S; ++d) {
        const float* pl = tile + d * N * DEPTH;
#pragma unroll 1
        for (int r0 = 0; r0 < N; r0 += N / DEPTH) {
          const int r = r0 + sub;
          const float v = pl[r * DEPTH + (ts ^ (r & (DEPTH - 1)))];
          if (ts < nt) cloud[((k * N + r) * S + d) * H + tb + ts] = v;
        }
      }
    }
    __syncthreads();  // the tile is read before the next one's steps overwrite it
  }
#pragma unroll
  for (int d = 0; d < S; ++d) state_end[p * S + d] = x[d];
  if (tid == 0) loglik[k] = ll;
}

}  // namespace pfk

int check_filter_args(const char* name, const VissmPfDesc* d, bool pointers, bool pointers_h) {
  VISSM_CHECK_ARG(pf::valid_n(d->N), "%s: N=%d particles (64, 128, 256, 512 or 1024)", name, d->N);
  VISSM_CHECK_ARG(d->K >= 0 && d->H >= 0 && d->t0 >= 0 && d->T_total >= 0, "%s: bad shape K=%d H=%d t0=%d T_total=%d",
                  name, d->K, d->H, d->t0, d->T_total);
  VISSM_CHECK_ARG(static_cast<int64_t>(d->K) * d->N < (int64_t{1} << 31), "%s: K N = %d %d reaches 2^31", name, d->K,
                  d->N);
  VISSM_CHECK_ARG(pointers, "%s: null pointer", name);
  VISSM_CHECK_ARG(d->H == 0 || pointers_h, "%s: null pointer (H > 0)", name);
  return VISSM_OK;
}

}  // namespace vissm

using namespace vissm;
using namespace vissm::pfk;

extern "C" int32_t vissm_particle_filter_lds_bytes(int32_t model, int32_t N) {
  if (!(model == VISSM_MODEL_AR || model == VISSM_MODEL_LV || model == VISSM_MODEL_FHN) || !pf::valid_n(N)) return 0;
  const int S = VISSM_MODEL_S(model), D = tile_depth(S, N);
  return 4 * S * N * D + 8 * N + 4 * S * N + 8 * D + 16 * (4 + 8 + 8);
}

namespace {

int run_filter(int proposal, const VissmPfDesc* d, uint64_t seed, uint64_t row0, const float* theta,
               const float* x_start, const float* obs, const float* obs_bin, const double* loglik_in, double* loglik,
               float* ll_inc, float* ess, float* state_end, float* cloud, uint64_t* q_trace, int32_t* anc_trace,
               void* stream) {
  // host arithmetic only, before any GPU call
  VISSM_CHECK_ARG(d, "particle_filter: null descriptor");
  VISSM_CHECK_ARG(d->model != VISSM_MODEL_SV,
                  "particle_filter: no observation model for SV (its first coordinate is the observed series)");
  VISSM_CHECK_ARG(d->model == VISSM_MODEL_AR || d->model == VISSM_MODEL_LV || d->model == VISSM_MODEL_FHN,
                  "particle_filter: unknown model %d", d->model);
  if (const int rc = check_filter_args("particle_filter", d, theta && x_start && loglik && state_end,
                                       obs && obs_bin && ll_inc && ess))
    return rc;
  const int S = VISSM_MODEL_S(d->model);
  VISSM_CHECK_ARG((static_cast<int64_t>(d->t0) + d->H) * S < (int64_t{1} << 31),
                  "particle_filter: (t0 + H) S = (%d + %d) %d reaches 2^31", d->t0, d->H, S);
  VISSM_CHECK_ARG(static_cast<int64_t>(d->t0) + d->H <= d->T_total,
                  "particle_filter: steps %d .. %d leave the %d observations", d->t0, d->t0 + d->H, d->T_total);
  // (the conditional degenerates at obs_std = 0; a NaN fails the first comparison, an infinity the second)
  VISSM_CHECK_ARG(proposal != kAdapted || (d->obs_std > 0.f && d->obs_std <= 3.4028234e38f),
                  "particle_filter: the adapted proposal needs a positive, finite obs_std, got %g",
                  static_cast<double>(d->obs_std));
  if (d->K == 0) return VISSM_OK;
  auto launch = [&](auto model, auto n, auto prop) {
    hipLaunchKernelGGL((particle_filter_kernel<decltype(model)::value, decltype(n)::value, decltype(prop)::value>),
                       dim3(d->K), dim3(d->N), 0, as_stream(stream), seed, row0, d->H, d->t0, d->T_total, d->dt,
                       d->obs_std, theta, x_start, obs, obs_bin, loglik_in, loglik, ll_inc, ess, state_end, cloud,
                       reinterpret_cast<unsigned long long*>(q_trace), anc_trace);
  };
  dispatch_model(d->model, [&](auto model) {
    dispatch_n(d->N, [&](auto n) {
      if (proposal == kAdapted) launch(model, n, std::integral_constant<int, kAdapted>{});
      else launch(model, n, std::integral_constant<int, kBootstrap>{});
    });
  });
  VISSM_CHECK_LAUNCH(proposal == kAdapted ? "particle_filter_adapted" : "particle_filter");
  return VISSM_OK;
}

}  // namespace

extern "C" int vissm_particle_filter(const VissmPfDesc* d, uint64_t seed, uint64_t row0, const float* theta,
                                     const float* x_start, const float* obs, const float* obs_bin,
                                     const double* loglik_in, double* loglik, float* ll_inc, float* ess,
                                     float* state_end, float* cloud, uint64_t* q_trace, int32_t* anc_trace,
                                     void* stream) {
  return run_filter(kBootstrap, d, seed, row0, theta, x_start, obs, obs_bin, loglik_in, loglik, ll_inc, ess, state_end,
                    cloud, q_trace, anc_trace, stream);
}

// the adapted filter declares the bootstrap kernel's arrays: the same LDS
extern "C" int32_t vissm_particle_filter_adapted_lds_bytes(int32_t model, int32_t N) {
  return vissm_particle_filter_lds_bytes(model, N);
}

extern "C" int vissm_particle_filter_adapted(const VissmPfDesc* d, uint64_t seed, uint64_t row0, const float* theta,
                                             const float* x_start, const float* obs, const float* obs_bin,
                                             const double* loglik_in, double* loglik, float* ll_inc, float* ess,
                                             float* state_end, float* cloud, uint64_t* q_trace, int32_t* anc_trace,
                                             void* stream) {
  return run_filter(kAdapted, d, seed, row0, theta, x_start, obs, obs_bin, loglik_in, loglik, ll_inc, ess, state_end,
                    cloud, q_trace, anc_trace, stream);
}
