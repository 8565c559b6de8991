// libvissm: forward simulation of the four SDEs (vissm_sde_simulate, include/vissm.h) -- posterior-predictive
// forecasts from per-sample theta and start states.  One lane per sample walks the serial Euler-Maruyama chain
// (sim_math.hpp, the step the ELBO's transition densities score); the normals come from the Philox / Box-Muller
// stream of vissm_normal_base, drawn in the kernel one group ahead of the step that consumes them, so the ten Philox
// rounds do not sit on the chain.
//
// Output is sample-major [B][S][H].  A lane that stored its own row would write 64 different cache lines per
// instruction, so each wave stages VISSM_SIM_TILE = 64 steps of its 64 samples in LDS -- one [64][64] plane per
// output coordinate -- and then writes the planes out row by row, the 64 lanes on consecutive steps of one sample:
// 256-byte segments.  Element (sample s, step t) of a plane lives at s * 64 + (t ^ s).  ds_write_b32 and ds_read_b32
// bank by (address / 4) % 32 within each 32-lane half: the step-loop write (lane = s, t fixed) and the row read
// (lane = t, s fixed) both see (t ^ s) & 31, distinct over the varying index, so neither conflicts and the plane
// needs no padding (4 planes of LV / FHN with observations = 64 KiB, the most one block may declare).
// A wave owns its planes (blocks are one wave), so the only synchronisation is a wave-level LDS fence.
#include "common.hpp"
#include "sim_math.hpp"

namespace vissm {
namespace {

constexpr int kTile = VISSM_SIM_TILE;
static_assert(kTile == 64, "a tile row is one wave-wide store of 64 consecutive steps");

// LDS writes of this wave's lanes become visible to its other lanes (DS operations of a wave complete in order)
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int MODEL, bool OBS>
__global__ __launch_bounds__(64) void sde_simulate_kernel(uint64_t seed, uint64_t row0, int B, int H, int t0, float dt,
                                                          float obs_std, const float* __restrict__ theta,
                                                          const float* __restrict__ x_start, float* __restrict__ xo,
                                                          float* __restrict__ yo, float* __restrict__ x_end) {
  constexpr int S = VISSM_MODEL_S(MODEL), P = VISSM_MODEL_P(MODEL);
  constexpr int NS = OBS ? 2 * S : S;  // normals per step = output planes
  const int lane = threadIdx.x;
  const int b0 = blockIdx.x * 64;      // the wave's first sample
  const int b = b0 + lane;
  const bool active = b < B;

  // an idle lane of the last wave walks a dummy chain (nothing of it is stored)
  float th[sim::kMaxP] = {0.f, 0.f, 0.f, 0.f, 0.f};
  float x[sim::kMaxS] = {0.f, 0.f}, y[sim::kMaxS] = {0.f, 0.f};
  if (active) {
#pragma unroll
    for (int i = 0; i < P; ++i) th[i] = theta[static_cast<size_t>(b) * P + i];
#pragma unroll
    for (int d = 0; d < S; ++d) x[d] = x_start[static_cast<size_t>(b) * S + d];
  }
  const sim::Par par = sim::prepare<MODEL>(th, dt);
  sim::start<MODEL>(x);

  const uint64_t row = row0 + static_cast<uint64_t>(b);
  const uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
  uint32_t j = static_cast<uint32_t>(t0) * NS;  // stream entry of the step's first normal ((t0 + H) NS < 2^31)
  uint32_t g = j >> 2;                          // its Philox group; NS divides 4, so a step never straddles two
  float cur[4], nxt[4];
  draw4(g, row, k0, k1, cur);
  draw4(g + 1, row, k0, k1, nxt);

#ifndef VISSM_SIM_DIRECT_STORE
  __shared__ float tile[NS * 64 * kTile];
  const int ns = min(64, B - b0);  // the wave's samples
#endif

  for (int tb = 0; tb < H; tb += kTile) {
    const int nt = min(kTile, H - tb);
    for (int tt = 0; tt < nt; ++tt) {
      const uint32_t q = j & 3u;
      float n[4];
      if constexpr (NS == 4) {
        n[0] = cur[0]; n[1] = cur[1]; n[2] = cur[2]; n[3] = cur[3];
      } else if constexpr (NS == 2) {
        n[0] = q ? cur[2] : cur[0];
        n[1] = q ? cur[3] : cur[1];
      } else {
        n[0] = q == 0 ? cur[0] : q == 1 ? cur[1] : q == 2 ? cur[2] : cur[3];
      }
      sim::advance<MODEL>(x, par, n, obs_std, OBS ? y : nullptr);
#ifndef VISSM_SIM_DIRECT_STORE
      const int at = lane * kTile + (tt ^ lane);
#pragma unroll
      for (int d = 0; d < S; ++d) {
        tile[d * 64 * kTile + at] = x[d];
        if constexpr (OBS) tile[(S + d) * 64 * kTile + at] = y[d];
      }
#else
      if (active) {
#pragma unroll
        for (int d = 0; d < S; ++d) {
          const size_t at = (static_cast<size_t>(b) * S + d) * H + tb + tt;
          xo[at] = x[d];
          if constexpr (OBS) yo[at] = y[d];
        }
      }
#endif
      j += NS;
      if ((j & 3u) == 0u) {  // wave-uniform: the next step opens a new group; draw the one after it now
#pragma unroll
        for (int i = 0; i < 4; ++i) cur[i] = nxt[i];
        ++g;
        draw4(g + 1, row, k0, k1, nxt);
      }
    }
#ifndef VISSM_SIM_DIRECT_STORE
    wave_lds_fence();
    // plane p, sample row s: lanes 0 .. nt-1 store steps tb .. tb+nt-1 of one output row
#pragma unroll
    for (int p = 0; p < NS; ++p) {
      float* __restrict__ out = (p < S ? xo : yo) + (static_cast<size_t>(b0) * S + (p % S)) * H + tb + lane;
      const float* pl = tile + p * 64 * kTile;
#pragma unroll 8
      for (int s = 0; s < ns; ++s) {
        const float v = pl[s * kTile + (lane ^ s)];
        if (lane < nt) out[static_cast<size_t>(s) * S * H] = v;
      }
    }
    wave_lds_fence();  // the rows are read before the next tile's steps overwrite them
#endif
  }
  if (active) {
#pragma unroll
    for (int d = 0; d < S; ++d) x_end[static_cast<size_t>(b) * S + d] = x[d];
  }
}

template <int MODEL, bool OBS>
void launch(const VissmSimDesc* d, uint64_t seed, uint64_t row0, const float* theta, const float* x_start, float* x,
            float* y, float* x_end, hipStream_t st) {
  hipLaunchKernelGGL((sde_simulate_kernel<MODEL, OBS>), dim3((d->B + 63) / 64), dim3(64), 0, st, seed, row0, d->B, d->H,
                     d->t0, d->dt, d->obs_std, theta, x_start, x, y, x_end);
}

}  // namespace
}  // namespace vissm

using namespace vissm;

extern "C" int vissm_sde_simulate(const VissmSimDesc* d, uint64_t seed, uint64_t row0, const float* theta,
                                  const float* x_start, float* x, float* y, float* x_end, void* stream) {
  VISSM_CHECK_ARG(d, "sde_simulate: null descriptor");
  VISSM_CHECK_ARG(d->model >= VISSM_MODEL_AR && d->model <= VISSM_MODEL_FHN, "sde_simulate: unknown model %d", d->model);
  VISSM_CHECK_ARG(d->B >= 0 && d->H >= 0 && d->t0 >= 0, "sde_simulate: bad shape B=%d H=%d t0=%d", d->B, d->H, d->t0);
  VISSM_CHECK_ARG(d->with_obs == 0 || d->with_obs == 1, "sde_simulate: with_obs=%d (0 or 1)", d->with_obs);
  VISSM_CHECK_ARG(!(d->with_obs && d->model == VISSM_MODEL_SV),
                  "sde_simulate: no observation model for SV (its first coordinate is the observed series)");
  const int S = VISSM_MODEL_S(d->model), NS = d->with_obs ? 2 * S : S;
  VISSM_CHECK_ARG(d->n_stream == NS, "sde_simulate: n_stream=%d, model %d with_obs=%d draws %d normals per step",
                  d->n_stream, d->model, d->with_obs, NS);
  VISSM_CHECK_ARG((static_cast<int64_t>(d->t0) + d->H) * NS < (int64_t{1} << 31),
                  "sde_simulate: (t0 + H) n_stream = (%d + %d) %d reaches 2^31", d->t0, d->H, NS);
  VISSM_CHECK_ARG(theta && x_start && x_end && (x || d->H == 0), "sde_simulate: null pointer");
  VISSM_CHECK_ARG(!d->with_obs || y || d->H == 0, "sde_simulate: null pointer (with_obs without y)");
  if (d->B == 0) return VISSM_OK;
  hipStream_t st = as_stream(stream);
  switch (d->model * 2 + d->with_obs) {
    case VISSM_MODEL_AR * 2: launch<VISSM_MODEL_AR, false>(d, seed, row0, theta, x_start, x, y, x_end, st); break;
    case VISSM_MODEL_AR * 2 + 1: launch<VISSM_MODEL_AR, true>(d, seed, row0, theta, x_start, x, y, x_end, st); break;
    case VISSM_MODEL_LV * 2: launch<VISSM_MODEL_LV, false>(d, seed, row0, theta, x_start, x, y, x_end, st); break;
    case VISSM_MODEL_LV * 2 + 1: launch<VISSM_MODEL_LV, true>(d, seed, row0, theta, x_start, x, y, x_end, st); break;
    case VISSM_MODEL_SV * 2: launch<VISSM_MODEL_SV, false>(d, seed, row0, theta, x_start, x, y, x_end, st); break;
    case VISSM_MODEL_FHN * 2: launch<VISSM_MODEL_FHN, false>(d, seed, row0, theta, x_start, x, y, x_end, st); break;
    default: launch<VISSM_MODEL_FHN, true>(d, seed, row0, theta, x_start, x, y, x_end, st); break;
  }
  VISSM_CHECK_LAUNCH("sde_simulate");
  return VISSM_OK;
}
