// libvissm: particle smoother of the AR, LV and FHN state-space models by forward filtering, backward simulation
// (vissm_particle_smooth, include/vissm.h) over the cloud vissm_particle_filter wrote.  The reference has no smoother:
// the backward weights restate its transition models (AR.py:172-176, lotka_volterra_partial.py:244-261,
// fitz_nag_NVP.py:243-255) through ps_math.hpp.
//
// A block owns filter k = blockIdx.y and the 64 trajectories blockIdx.x 64 .. + 63 of its M, one per lane of each of its
// NW = min(4, N / 64) waves; wave w scores the particles [w N / NW, (w + 1) N / NW) for all 64 trajectories, so K M / 64
// blocks put K M NW / 64 waves on the machine.  The block walks t from H - 1 down.  Per step, with xt the lane's state
// at t + 1:
//   prep     the per-particle part of all N particles (ps::particle), once per block into LDS
//   pass 1   the maximum of logw over the wave's particles: every lane reads the same particle, an LDS broadcast;
//            barrier; m = the maximum of the waves' maxima (exact in any order)
//   pass 2   the sum of q over each run of 64 of the wave's particles, in registers: N / NW exps per lane;
//            barrier; W = the waves' sums, and the cumulative sum at the wave's first particle
//   pass 3   the wave whose range holds tau finds the run that does from its run sums, then C_i inside that run only:
//            64 pair evaluations and exps, each lane in its own run; it gathers the chosen state
//            barrier; every wave takes the new xt
// so a pair costs two evaluations and 1 + 64 / N exps.  Everything after the exp is integer and C is defined in
// particle order: the chosen particle depends on no launch geometry.  No atomics, no workspace: two launches are
// bitwise equal, and trajectory (k, j) depends on (seed, row0 + k N + j, theta_k, filter k's cloud, x_next[k, j]) only.
//
// Cloud staging: the filter's cloud is sample-major [K N][S][H].  For each tile of DEPTH steps the block reads row
// segments of DEPTH consecutive steps (DEPTH lanes on one row) and stores plane d, particle i, step t at
// i DEPTH + (t ^ (i mod DEPTH)) -- particle.hip's swizzle mirrored: the 64 lanes of a store cover 64 consecutive
// words, and the per-step read (lane i, fixed t) is conflict-free at DEPTH = 32 and 64 / DEPTH-way below it (it is
// read once per step and particle).  The chosen states and indices are staged the same way and leave as row segments
// of DEPTH consecutive steps.  DEPTH = clamp(16 KiB / (4 S N), 4, 32): the pair loop is three orders of magnitude more
// work than the staging, so the tile is kept small enough for two waves and more per SIMD instead of long segments:
//                N = 64   128   256   512   1024
//   AR             32    32    16     8      4
//   LV / FHN       32    16     8     4      4
// (segments below 128 bytes everywhere but at DEPTH = 32; 16 bytes at DEPTH = 4: a 64-byte line is then fetched by four
// consecutive tiles, from L2 after the first).  LDS per block = 4 S N DEPTH (tile) + 4 L N (prep; L = 1 AR, 6 LV,
// 2 FHN) + 4 (S + 1) 64 DEPTH (paths, idx) + 768 NW (the waves' maxima and sums) + 256 (S + 1) (the chosen state):
// at most 64,256 bytes (LV, N = 1024; vissm_particle_smooth_lds_bytes), two blocks and eight waves per CU.
#include "common.hpp"
#include "ps_math.hpp"

namespace vissm {
namespace psk {

constexpr int kTileBytes = 16 * 1024;
constexpr int kLanes = 64;

constexpr int tile_depth(int S, int N) {
  const int d = kTileBytes / (4 * S * N);
  return d > 32 ? 32 : d < 4 ? 4 : d;
}

// waves per block: each scores N / NW particles
constexpr int block_waves(int N) { return N / 64 < 4 ? N / 64 : 4; }

template <int MODEL, int N>
__global__ __launch_bounds__(kLanes* block_waves(N)) void particle_smooth_kernel(
    uint64_t seed, uint64_t row0, int M, int H, int t0, float dt, const float* __restrict__ theta,
    const float* __restrict__ cloud, const float* __restrict__ x_next, float* __restrict__ paths,
    float* __restrict__ x_first, int32_t* __restrict__ idx_out, unsigned long long* __restrict__ q_trace) {
  constexpr int S = VISSM_MODEL_S(MODEL), P = VISSM_MODEL_P(MODEL), L = ps::prep_len(MODEL);
  constexpr int DEPTH = tile_depth(S, N), NW = block_waves(N), NT = kLanes * NW;
  constexpr int CW = N / 64 / NW;  // runs of 64 particles per wave
  static_assert(DEPTH >= 4 && DEPTH <= 32 && (DEPTH & (DEPTH - 1)) == 0, "tile depth");
  static_assert(CW >= 1 && CW * NW * 64 == N && N % (NT / DEPTH) == 0, "particles per wave");
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const size_t k = blockIdx.y;
  const int j0 = blockIdx.x * kLanes, j = j0 + lane;  // M is a multiple of 64: every lane has a trajectory
  const size_t traj = k * M + j;

  __shared__ float tile[S * N * DEPTH];
  __shared__ float prep[L * N];
  __shared__ float opath[S * kLanes * DEPTH];
  __shared__ int32_t oidx[kLanes * DEPTH];
  __shared__ float wmax[NW][kLanes];
  __shared__ uint64_t wsum[NW][kLanes];
  __shared__ float xsel[S][kLanes];
  __shared__ int32_t isel[kLanes];

  float th[sim::kMaxP] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < P; ++i) th[i] = theta[k * P + i];
  const ps::Par par = ps::prepare<MODEL>(th, dt);

  float xt[sim::kMaxS] = {0.f, 0.f};
  const bool have_next = x_next != nullptr;
  if (have_next) {
#pragma unroll
    for (int d = 0; d < S; ++d) xt[d] = x_next[traj * S + d];
  }
  const uint64_t row = row0 + k * N + static_cast<uint64_t>(j);
  const int i0 = wv * CW * 64;  // the wave's first particle

  // the weight of particle i for this lane's target
  auto logw = [&](int i) -> float {
    ps::Prep r;
#pragma unroll
    for (int c = 0; c < L; ++c) r.c[c] = prep[c * N + i];
    return ps::pair_logw<MODEL>(r, par, xt);
  };

  const int ts = tid & (DEPTH - 1), sub = tid / DEPTH;
  for (int tb = (H - 1) / DEPTH * DEPTH; tb >= 0; tb -= DEPTH) {
    const int nt = min(DEPTH, H - tb);
    // stage the cloud's steps tb .. tb + nt - 1: NT / DEPTH rows at once, DEPTH lanes on one row's consecutive steps
#pragma unroll
    for (int d = 0; d < S; ++d) {
      float* pl = tile + d * N * DEPTH;
#pragma unroll 4
      for (int r0 = 0; r0 < N; r0 += NT / DEPTH) {
        const int r = r0 + sub;
        const float v = ts < nt ? cloud[((k * N + r) * S + d) * H + tb + ts] : 0.f;
        pl[r * DEPTH + (ts ^ (r & (DEPTH - 1)))] = v;
      }
    }
    __syncthreads();

    for (int tt = nt - 1; tt >= 0; --tt) {
      const int t = tb + tt;
      const bool terminal = t == H - 1 && !have_next;
      // the per-particle part of this step, shared by the block's trajectories
#pragma unroll 1
      for (int i = tid; i < N; i += NT) {
        float x[sim::kMaxS] = {0.f, 0.f};
        const int at = i * DEPTH + (tt ^ (i & (DEPTH - 1)));
#pragma unroll
        for (int d = 0; d < S; ++d) x[d] = tile[d * N * DEPTH + at];
        ps::Prep r = ps::particle<MODEL>(x, par);
        if (terminal) {  // an all-zero prep and a zero target give logw = 0, a NaN prep NaN: ps::terminal_logw
          const float z = ps::terminal_logw(r.c[0]);
#pragma unroll
          for (int c = 0; c < L; ++c) r.c[c] = z;
        }
#pragma unroll
        for (int c = 0; c < L; ++c) prep[c * N + i] = r.c[c];
      }
      if (terminal) {
#pragma unroll
        for (int d = 0; d < S; ++d) xt[d] = 0.f;
      }
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
          const int at = idx * DEPTH + (tt ^ (idx & (DEPTH - 1)));
#pragma unroll
          for (int d = 0; d < S; ++d) xsel[d][lane] = tile[d * N * DEPTH + at];
          isel[lane] = idx;
        }
      } else if (wv == 0) {  // no live particle, or a NaN target
#pragma unroll
        for (int d = 0; d < S; ++d) xsel[d][lane] = sim::quiet_nan();
        isel[lane] = -1;
      }
      __syncthreads();
#pragma unroll
      for (int d = 0; d < S; ++d) xt[d] = xsel[d][lane];
      if (wv == 0) {
        const int ot = lane * DEPTH + (tt ^ (lane & (DEPTH - 1)));
#pragma unroll
        for (int d = 0; d < S; ++d) opath[d * kLanes * DEPTH + ot] = xt[d];
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
#pragma unroll
          for (int d = 0; d < S; ++d) paths[(orow * S + d) * H + tb + ls] = opath[d * kLanes * DEPTH + ot];
          if (idx_out) idx_out[orow * H + tb + ls] = oidx[ot];
        }
      }
    }
    __syncthreads();  // the tiles are read before the next one overwrites them
  }
  if (wv == 0) {
#pragma unroll
    for (int d = 0; d < S; ++d) x_first[traj * S + d] = xt[d];
  }
}

}  // namespace psk
}  // namespace vissm

using namespace vissm;
using namespace vissm::psk;

extern "C" int32_t vissm_particle_smooth_lds_bytes(int32_t model, int32_t N, int32_t M) {
  if (!(model == VISSM_MODEL_AR || model == VISSM_MODEL_LV || model == VISSM_MODEL_FHN) || !pf::valid_n(N) ||
      !ps::valid_m(M, N))
    return 0;
  const int S = VISSM_MODEL_S(model), D = tile_depth(S, N);
  return 4 * S * N * D + 4 * ps::prep_len(model) * N + 4 * (S + 1) * kLanes * D + 768 * block_waves(N) +
         256 * (S + 1);
}

extern "C" int vissm_particle_smooth(const VissmPsDesc* d, uint64_t seed, uint64_t row0, const float* theta,
                                     const float* cloud, const float* x_next, float* paths, float* x_first,
                                     int32_t* idx, uint64_t* q_trace, void* stream) {
  // host arithmetic only, before any GPU call
  VISSM_CHECK_ARG(d, "particle_smooth: null descriptor");
  VISSM_CHECK_ARG(d->model != VISSM_MODEL_SV,
                  "particle_smooth: no particle filter for SV (its first coordinate is the observed series)");
  VISSM_CHECK_ARG(d->model == VISSM_MODEL_AR || d->model == VISSM_MODEL_LV || d->model == VISSM_MODEL_FHN,
                  "particle_smooth: unknown model %d", d->model);
  VISSM_CHECK_ARG(pf::valid_n(d->N), "particle_smooth: N=%d particles (64, 128, 256, 512 or 1024)", d->N);
  VISSM_CHECK_ARG(ps::valid_m(d->M, d->N), "particle_smooth: M=%d trajectories (a power of two, 64 <= M <= N = %d)",
                  d->M, d->N);
  VISSM_CHECK_ARG(d->K >= 0 && d->K <= 65535 && d->H >= 1 && d->t0 >= 0,
                  "particle_smooth: bad shape K=%d (0 .. 65535) H=%d (>= 1) t0=%d", d->K, d->H, d->t0);
  VISSM_CHECK_ARG(static_cast<int64_t>(d->t0) + d->H < (int64_t{1} << 31),
                  "particle_smooth: t0 + H = %d + %d reaches 2^31", d->t0, d->H);
  VISSM_CHECK_ARG(theta && cloud && paths && x_first, "particle_smooth: null pointer");
  if (d->K == 0) return VISSM_OK;
  dispatch_model(d->model, [&](auto model) {
    dispatch_n(d->N, [&](auto n) {
      constexpr int N = decltype(n)::value;
      hipLaunchKernelGGL((particle_smooth_kernel<decltype(model)::value, N>), dim3(d->M / kLanes, d->K),
                         dim3(kLanes * block_waves(N)), 0, as_stream(stream), seed, row0, d->M, d->H, d->t0, d->dt,
                         theta, cloud, x_next, paths, x_first, idx, reinterpret_cast<unsigned long long*>(q_trace));
    });
  });
  VISSM_CHECK_LAUNCH("particle_smooth");
  return VISSM_OK;
}
