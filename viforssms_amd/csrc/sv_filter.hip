// libvissm: particle filter and smoother of the stochastic-volatility model (vissm_sv_filter, vissm_sv_smooth;
// include/vissm.h).  vissm_particle_filter refuses SV because it has no obs_std / obs_bin observation model; here the
// observed series y is the first coordinate of the Euler-Maruyama state and the particle is the latent h alone
// (svf_math.hpp; the reference's model: SV_dense.py:203-223).  The reference has neither a filter nor a smoother.
//
// Filter: particle.hip's PROPOSAL = kAdapted body with S = 1 -- one block per filter, one particle per lane, the same
// four barriers A-D around the integer pipeline of pf_math.hpp, AR's Philox stream (n_stream = 1, drawn one group
// ahead) and AR's swizzled LDS tile (DEPTH = 64 up to N = 512, 32 at N = 1024).  Every step is observed: step ta scores
// the *pre-step* h on (y[ta], y[ta + 1]) (svf::state_logw), resamples, gathers the ancestor's h through LDS and moves it
// with the lane's own normal (svf::move: the prior transition is the exact conditional, because the move does not
// depend on y).  Cloud column t holds h after the move, an equally weighted sample of p(h_ta+1 | y_0:ta+1).
// LDS per block = 4 N DEPTH (tile) + 8 N (C) + 4 N (gather) + 8 DEPTH + 320: at most 143,936 bytes.
//
// Smoother: smooth.hip's geometry with S = 1 and a per-particle part of two floats -- a block owns 64 trajectories of
// one filter, up to four waves share out the particles, three passes per step, integer selection on counter word 2.
// Column c (absolute ca = t0 + c) holds h_ca+1; because y_ca+2 depends on h_ca+1 the backward weight is
//   logw_i = log f(xt | h_i) + svf::state_logw(h_i, y[ca + 1], y[ca + 2])
// and the second term goes into the once-per-step LDS prep, so the pair loop stays one fma chain and one exp.
// LDS per block = 4 N DEPTH (tile; smooth.hip's AR depths) + 8 N (prep) + 512 DEPTH (paths, idx) + 768 NW + 512.
#include "common.hpp"
#include "svf_math.hpp"

namespace vissm {
namespace svk {

constexpr int kP = VISSM_MODEL_P(VISSM_MODEL_SV);

// ---- filter -------------------------------------------------------------------------------------------------------
constexpr int kTileBytes = 128 * 1024;

constexpr int tile_depth(int N) {
  const int d = kTileBytes / (4 * N);
  return d > 64 ? 64 : d;
}

template <int N>
__global__ __launch_bounds__(N) void sv_filter_kernel(
    uint64_t seed, uint64_t row0, int H, int t0, float dt, const float* __restrict__ theta,
    const float* __restrict__ x_start, const float* __restrict__ obs, const double* __restrict__ loglik_in,
    double* __restrict__ loglik, float* __restrict__ ll_inc, float* __restrict__ ess_out,
    float* __restrict__ state_end, float* __restrict__ cloud, unsigned long long* __restrict__ q_trace,
    int32_t* __restrict__ anc_trace) {
  constexpr int NW = N / 64, LOG2N = pf::log2_of(N);
  constexpr int DEPTH = tile_depth(N);
  static_assert(DEPTH >= 16 && (DEPTH & (DEPTH - 1)) == 0 && N % DEPTH == 0, "tile depth");
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const size_t k = blockIdx.x;
  const size_t p = k * N + tid;  // the particle's row in the [K N] arrays

  __shared__ float tile[N * DEPTH];
  __shared__ uint64_t Cs[N];
  __shared__ float xs[N];
  __shared__ float ll_tile[DEPTH], ess_tile[DEPTH];
  __shared__ float wmax[16];
  __shared__ uint64_t wtot[16];
  __shared__ double wsq[16];

  float th[sim::kMaxP] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < kP; ++i) th[i] = theta[k * kP + i];
  const sim::Par par = sim::prepare<VISSM_MODEL_SV>(th, dt);
  float h = x_start[p];
  if (!__builtin_isfinite(h)) h = sim::quiet_nan();

  // block-uniform: a filter that died in an earlier call stays dead
  double ll = loglik_in ? loglik_in[k] : 0.0;
  if (ll == -INFINITY) h = sim::quiet_nan();

  const uint64_t frow = row0 + k * N;  // the filter's first Philox row: keys its resampling integers
  const uint64_t row = frow + static_cast<uint64_t>(tid);
  const uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
  uint32_t j = static_cast<uint32_t>(t0);  // stream entry of the step's normal (t0 + H < 2^31)
  uint32_t g = j >> 2;                     // its Philox group
  float cur[4], nxt[4];
  draw4(g, row, k0, k1, cur);
  draw4(g + 1, row, k0, k1, nxt);

  for (int tb = 0; tb < H; tb += DEPTH) {
    const int nt = min(DEPTH, H - tb);
    for (int tt = 0; tt < nt; ++tt) {
      const int ta = t0 + tb + tt;  // absolute step
      const uint32_t qd = j & 3u;
      const float n = qd == 0 ? cur[0] : qd == 1 ? cur[1] : qd == 2 ? cur[2] : cur[3];

      // every thread reads the same addresses: block-uniform
      const svf::Obs ob = svf::obs_prep(obs[ta], obs[static_cast<size_t>(ta) + 1], par);

      float inc = sim::quiet_nan(), es = sim::quiet_nan();
      const bool ok = __builtin_isfinite(h);
      const float lw = svf::state_logw(h, ob);
      const float wm = wave_max(lw);
      if (lane == 0) wmax[wid] = wm;
      xs[tid] = h;
      __syncthreads();  // A
      float m = wmax[0];
#pragma unroll
      for (int w = 1; w < NW; ++w) m = fmaxf(m, wmax[w]);
      const uint64_t q = pf::quantise(lw, m, ok);
      const uint64_t c = wave_scan(q, lane);
      const double qq = static_cast<double>(q);
      const double s2 = wave_sum(qq * qq);
      if (lane == 63) wtot[wid] = c;
      if (lane == 0) wsq[wid] = s2;
      __syncthreads();  // B
      uint64_t before = 0, W = 0;
      double Q2 = 0.0;
#pragma unroll 2  // (particle.hip: all sixteen partials in flight cost the 1024-lane block registers)
      for (int w = 0; w < NW; ++w) {
        if (w < wid) before += wtot[w];
        W += wtot[w];
        Q2 += wsq[w];
      }
      Cs[tid] = c + before;
      __syncthreads();  // C
      int anc = tid;
      if (W > 0) {  // (a dead filter has every q = 0)
        const uint32_t U = pf::resample_u(seed, static_cast<uint32_t>(ta), frow);
        anc = pf::ancestor(Cs, N, pf::threshold(static_cast<uint32_t>(tid), U, W, LOG2N));
        anc = min(anc, N - 1);  // tau < W = C[N - 1]: never taken
        h = svf::move(xs[anc], par, n);
        const double li = pf::ll_increment(m, W, N);
        ll += li;
        inc = static_cast<float>(li);
        es = static_cast<float>(pf::ess(W, Q2));
      } else {  // no live particle with a weight: the filter is dead from here on
        ll = -INFINITY;
        h = sim::quiet_nan();
      }
      __syncthreads();  // D
      if (q_trace) q_trace[(k * H + tb + tt) * N + tid] = q;
      if (anc_trace) anc_trace[(k * H + tb + tt) * N + tid] = anc;
      if (tid == 0) {
        ll_tile[tt] = inc;
        ess_tile[tt] = es;
      }
      if (cloud) tile[tid * DEPTH + (tt ^ (tid & (DEPTH - 1)))] = h;
      ++j;
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
#pragma unroll 1
      for (int r0 = 0; r0 < N; r0 += N / DEPTH) {
        const int r = r0 + sub;
        const float v = tile[r * DEPTH + (ts ^ (r & (DEPTH - 1)))];
        if (ts < nt) cloud[(k * N + r) * H + tb + ts] = v;
      }
    }
    __syncthreads();  // the tile is read before the next one's steps overwrite it
  }
  state_end[p] = h;
  if (tid == 0) loglik[k] = ll;
}

// ---- smoother -----------------------------------------------------------------------------------------------------
constexpr int kSmoothTileBytes = 16 * 1024;
constexpr int kLanes = 64;

constexpr int smooth_depth(int N) {
  const int d = kSmoothTileBytes / (4 * N);
  return d > 32 ? 32 : d < 4 ? 4 : d;
}

// waves per block: each scores N / NW particles
constexpr int block_waves(int N) { return N / 64 < 4 ? N / 64 : 4; }

template <int N>
__global__ __launch_bounds__(kLanes* block_waves(N)) void sv_smooth_kernel(
    uint64_t seed, uint64_t row0, int M, int H, int t0, float dt, const float* __restrict__ theta,
    const float* __restrict__ cloud, const float* __restrict__ obs, const float* __restrict__ x_next,
    float* __restrict__ paths, float* __restrict__ x_first, int32_t* __restrict__ idx_out,
    unsigned long long* __restrict__ q_trace) {
  constexpr int DEPTH = smooth_depth(N), NW = block_waves(N), NT = kLanes * NW;
  constexpr int CW = N / 64 / NW;  // runs of 64 particles per wave
  static_assert(DEPTH >= 4 && DEPTH <= 32 && (DEPTH & (DEPTH - 1)) == 0, "tile depth");
  static_assert(CW >= 1 && CW * NW * 64 == N && N % (NT / DEPTH) == 0, "particles per wave");
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const size_t k = blockIdx.y;
  const int j0 = blockIdx.x * kLanes, j = j0 + lane;  // M is a multiple of 64: every lane has a trajectory
  const size_t traj = k * M + j;

  __shared__ float tile[N * DEPTH];
  __shared__ float prep[2 * N];
  __shared__ float opath[kLanes * DEPTH];
  __shared__ int32_t oidx[kLanes * DEPTH];
  __shared__ float wmax[NW][kLanes];
  __shared__ uint64_t wsum[NW][kLanes];
  __shared__ float xsel[kLanes];
  __shared__ int32_t isel[kLanes];

  float th[sim::kMaxP] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < kP; ++i) th[i] = theta[k * kP + i];
  const svf::SPar par = svf::sprepare(th, dt);

  const bool have_next = x_next != nullptr;
  float xt = have_next ? x_next[traj] : 0.f;
  const uint64_t row = row0 + k * N + static_cast<uint64_t>(j);
  const int i0 = wv * CW * 64;  // the wave's first particle

  // the weight of particle i for this lane's target
  auto logw = [&](int i) -> float {
    svf::Prep r;
    r.mean = prep[i];
    r.off = prep[N + i];
    return svf::pair_logw(r, par, xt);
  };

  const int ts = tid & (DEPTH - 1), sub = tid / DEPTH;
  for (int tb = (H - 1) / DEPTH * DEPTH; tb >= 0; tb -= DEPTH) {
    const int nt = min(DEPTH, H - tb);
    // stage the cloud's columns tb .. tb + nt - 1: NT / DEPTH rows at once, DEPTH lanes on one row's consecutive steps
#pragma unroll 4
    for (int r0 = 0; r0 < N; r0 += NT / DEPTH) {
      const int r = r0 + sub;
      const float v = ts < nt ? cloud[(k * N + r) * H + tb + ts] : 0.f;
      tile[r * DEPTH + (ts ^ (r & (DEPTH - 1)))] = v;
    }
    __syncthreads();

    for (int tt = nt - 1; tt >= 0; --tt) {
      const int t = tb + tt;
      const bool terminal = t == H - 1 && !have_next;
      // the per-particle part of this column, shared by the block's trajectories; the terminal column reads no
      // observation (y[ca + 2] may lie past the series)
      svf::Obs ob;
      ob.a = ob.c = 0.f;
      if (!terminal) {
        const size_t ca = static_cast<size_t>(t0) + t;
        ob = svf::obs_prep(obs[ca + 1], obs[ca + 2], par.p);
      }
#pragma unroll 1
      for (int i = tid; i < N; i += NT) {
        const float hi = tile[i * DEPTH + (tt ^ (i & (DEPTH - 1)))];
        svf::Prep r = svf::particle(hi, ob, par);
        if (terminal) r.mean = r.off = ps::terminal_logw(r.mean);  // zero prep, zero target: logw = 0; NaN stays NaN
        prep[i] = r.mean;
        prep[N + i] = r.off;
      }
      if (terminal) xt = 0.f;
      __syncthreads();

      // pass 1: the maximum over the live particles
      float m = -INFINITY;
#pragma unroll 8
      for (int i = 0; i < CW * 64; ++i) m = ps::max_live(m, logw(i0 + i));
      if constexpr (NW > 1) {
        wmax[wv][lane] = m;
        __syncthreads();
        m = wmax[0][lane];
#pragma unroll
        for (int w = 1; w < NW; ++w) m = ps::max_live(m, wmax[w][lane]);
      }

      // pass 2: the sums of the wave's runs of 64 particles; W and the cumulative sum before the wave's first particle
      uint64_t cs[CW];
      uint64_t mine = 0;
#pragma unroll
      for (int c = 0; c < CW; ++c) {
        uint64_t s = 0;
#pragma unroll 4
        for (int ii = 0; ii < 64; ++ii) s += pf::quantise(logw(i0 + c * 64 + ii), m, true);
        cs[c] = s;
        mine += s;
      }
      uint64_t W = mine, before = 0;
      if constexpr (NW > 1) {
        wsum[wv][lane] = mine;
        __syncthreads();
        W = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          const uint64_t v = wsum[w][lane];
          if (w < wv) before += v;
          W += v;
        }
      }
      if (q_trace) {  // tests only
        unsigned long long* qt = q_trace + ((k * H + t) * M + j) * N + i0;
#pragma unroll 1
        for (int i = 0; i < CW * 64; ++i) qt[i] = pf::quantise(logw(i0 + i), m, true);
      }

      int idx = -1;
      if (W > 0) {
        const uint64_t tau = ps::threshold(ps::select_u(seed, static_cast<uint32_t>(t0 + t), row), W);
        if (before <= tau && tau < before + mine) {  // tau < W: exactly one wave per lane
          // the run that holds tau: every C_i of an earlier run is <= base <= tau, every one of a later run > tau
          uint64_t cum = before, base = before;
          int c0 = 0;
#pragma unroll
          for (int c = 0; c < CW; ++c) {
            cum += cs[c];
            if (cum <= tau) {
              base = cum;
              c0 = c + 1;
            }
          }
          c0 = min(c0, CW - 1);  // tau < before + mine = the last cum: never taken
          idx = i0 + c0 * 64;
          uint64_t C = base;
#pragma unroll 4
          for (int ii = 0; ii < 64; ++ii) {
            C += pf::quantise(logw(i0 + c0 * 64 + ii), m, true);
            idx += C <= tau ? 1 : 0;
          }
          idx = min(idx, N - 1);  // never taken
          xsel[lane] = tile[idx * DEPTH + (tt ^ (idx & (DEPTH - 1)))];
          isel[lane] = idx;
        }
      } else if (wv == 0) {  // no live particle, or a NaN target
        xsel[lane] = sim::quiet_nan();
        isel[lane] = -1;
      }
      __syncthreads();
      xt = xsel[lane];
      if (wv == 0) {
        const int ot = lane * DEPTH + (tt ^ (lane & (DEPTH - 1)));
        opath[ot] = xt;
        oidx[ot] = isel[lane];
      }
      __syncthreads();  // the step's prep and choice are read before the next step overwrites them
    }

    // write the tile's chosen states and indices out as row segments of DEPTH consecutive steps
    if (wv == 0) {
      const int ls = lane & (DEPTH - 1), lsub = lane / DEPTH;
#pragma unroll
      for (int l0 = 0; l0 < kLanes; l0 += kLanes / DEPTH) {
        const int l = l0 + lsub;
        const int ot = l * DEPTH + (ls ^ (l & (DEPTH - 1)));
        if (ls < nt) {
          const size_t orow = k * M + j0 + l;
          paths[orow * H + tb + ls] = opath[ot];
          if (idx_out) idx_out[orow * H + tb + ls] = oidx[ot];
        }
      }
    }
    __syncthreads();  // the tiles are read before the next one overwrites them
  }
  if (wv == 0) x_first[traj] = xt;
}

}  // namespace svk
}  // namespace vissm

using namespace vissm;
using namespace vissm::svk;

extern "C" int32_t vissm_sv_filter_lds_bytes(int32_t N) {
  if (!pf::valid_n(N)) return 0;
  const int D = tile_depth(N);
  return 4 * N * D + 8 * N + 4 * N + 8 * D + 16 * (4 + 8 + 8);
}

extern "C" int vissm_sv_filter(const VissmPfDesc* d, uint64_t seed, uint64_t row0, const float* theta,
                               const float* x_start, const float* obs, const double* loglik_in, double* loglik,
                               float* ll_inc, float* ess, float* state_end, float* cloud, uint64_t* q_trace,
                               int32_t* anc_trace, void* stream) {
  // host arithmetic only, before any GPU call
  VISSM_CHECK_ARG(d, "sv_filter: null descriptor");
  VISSM_CHECK_ARG(d->model == VISSM_MODEL_SV, "sv_filter: model %d is not SV (vissm_particle_filter has the others)",
                  d->model);
  if (const int rc = check_filter_args("sv_filter", d, theta && x_start && loglik && state_end, obs && ll_inc && ess))
    return rc;
  VISSM_CHECK_ARG(static_cast<int64_t>(d->t0) + d->H < (int64_t{1} << 31), "sv_filter: t0 + H = %d + %d reaches 2^31",
                  d->t0, d->H);
  VISSM_CHECK_ARG(static_cast<int64_t>(d->t0) + d->H <= d->T_total,
                  "sv_filter: steps %d .. %d leave the %d transitions of the series", d->t0, d->t0 + d->H, d->T_total);
  // (a NaN fails the first comparison, an infinity the second)
  VISSM_CHECK_ARG(d->dt > 0.f && d->dt <= 3.4028234e38f, "sv_filter: dt must be positive and finite, got %g",
                  static_cast<double>(d->dt));
  if (d->K == 0) return VISSM_OK;
  dispatch_n(d->N, [&](auto n) {
    hipLaunchKernelGGL((sv_filter_kernel<decltype(n)::value>), dim3(d->K), dim3(d->N), 0, as_stream(stream), seed, row0,
                       d->H, d->t0, d->dt, theta, x_start, obs, loglik_in, loglik, ll_inc, ess, state_end, cloud,
                       reinterpret_cast<unsigned long long*>(q_trace), anc_trace);
  });
  VISSM_CHECK_LAUNCH("sv_filter");
  return VISSM_OK;
}

extern "C" int32_t vissm_sv_smooth_lds_bytes(int32_t N, int32_t M) {
  if (!pf::valid_n(N) || !ps::valid_m(M, N)) return 0;
  const int D = smooth_depth(N);
  return 4 * N * D + 8 * N + 8 * kLanes * D + 768 * block_waves(N) + 512;
}

extern "C" int vissm_sv_smooth(const VissmPsDesc* d, uint64_t seed, uint64_t row0, const float* theta,
                               const float* cloud, const float* obs, int32_t T_total, const float* x_next, float* paths,
                               float* x_first, int32_t* idx, uint64_t* q_trace, void* stream) {
  // host arithmetic only, before any GPU call
  VISSM_CHECK_ARG(d, "sv_smooth: null descriptor");
  VISSM_CHECK_ARG(d->model == VISSM_MODEL_SV, "sv_smooth: model %d is not SV (vissm_particle_smooth has the others)",
                  d->model);
  VISSM_CHECK_ARG(pf::valid_n(d->N), "sv_smooth: N=%d particles (64, 128, 256, 512 or 1024)", d->N);
  VISSM_CHECK_ARG(ps::valid_m(d->M, d->N), "sv_smooth: M=%d trajectories (a power of two, 64 <= M <= N = %d)", d->M,
                  d->N);
  VISSM_CHECK_ARG(d->K >= 0 && d->K <= 65535 && d->H >= 1 && d->t0 >= 0 && T_total >= 0,
                  "sv_smooth: bad shape K=%d (0 .. 65535) H=%d (>= 1) t0=%d T_total=%d", d->K, d->H, d->t0, T_total);
  VISSM_CHECK_ARG(static_cast<int64_t>(d->t0) + d->H < (int64_t{1} << 31), "sv_smooth: t0 + H = %d + %d reaches 2^31",
                  d->t0, d->H);
  // column c with a next state reads y[t0 + c + 2]: the last such column is H - 1 with x_next, H - 2 without
  VISSM_CHECK_ARG(static_cast<int64_t>(d->t0) + d->H + (x_next ? 1 : 0) <= T_total,
                  "sv_smooth: columns %d .. %d %s a next state need y[%lld] of a series of %d transitions", d->t0,
                  d->t0 + d->H - 1, x_next ? "with" : "without",
                  static_cast<long long>(d->t0) + d->H + (x_next ? 1 : 0), T_total);
  VISSM_CHECK_ARG(d->dt > 0.f && d->dt <= 3.4028234e38f, "sv_smooth: dt must be positive and finite, got %g",
                  static_cast<double>(d->dt));
  VISSM_CHECK_ARG(theta && cloud && obs && paths && x_first, "sv_smooth: null pointer");
  if (d->K == 0) return VISSM_OK;
  dispatch_n(d->N, [&](auto n) {
    constexpr int N = decltype(n)::value;
    hipLaunchKernelGGL((sv_smooth_kernel<N>), dim3(d->M / kLanes, d->K), dim3(kLanes * block_waves(N)), 0,
                       as_stream(stream), seed, row0, d->M, d->H, d->t0, d->dt, theta, cloud, obs, x_next, paths,
                       x_first, idx, reinterpret_cast<unsigned long long*>(q_trace));
  });
  VISSM_CHECK_LAUNCH("sv_smooth");
  return VISSM_OK;
}
