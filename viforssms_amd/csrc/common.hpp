// Shared helpers of libvissm: error state, launch checking, Philox RNG,
// wave/block reductions.  gfx950 only (wave64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <cstdio>
#include <type_traits>

#include "../../include/vissm.h"
#include "rng_math.hpp"

namespace vissm {

void set_error(const char* fmt, ...);

#define VISSM_CHECK_ARG(cond, ...)        \
  do {                                    \
    if (!(cond)) {                        \
      ::vissm::set_error(__VA_ARGS__);    \
      return VISSM_EINVAL;                \
    }                                     \
  } while (0)

#define VISSM_CHECK_LAUNCH(what)                                               \
  do {                                                                         \
    hipError_t e_ = hipGetLastError();                                         \
    if (e_ != hipSuccess) {                                                    \
      ::vissm::set_error("%s: %s", what, hipGetErrorString(e_));               \
      return VISSM_ELAUNCH;                                                    \
    }                                                                          \
  } while (0)

static inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

static inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// The particle kernels are templates on the particle count N (64, 128, 256, 512 or 1024: pf::valid_n, checked by the
// caller) and on the model (AR, LV or FHN, checked by the caller): f gets the value as a std::integral_constant.
template <class F>
void dispatch_n(int N, F&& f) {
  switch (N) {
    case 64: f(std::integral_constant<int, 64>{}); break;
    case 128: f(std::integral_constant<int, 128>{}); break;
    case 256: f(std::integral_constant<int, 256>{}); break;
    case 512: f(std::integral_constant<int, 512>{}); break;
    default: f(std::integral_constant<int, 1024>{}); break;
  }
}

template <class F>
void dispatch_model(int model, F&& f) {
  switch (model) {
    case VISSM_MODEL_AR: f(std::integral_constant<int, VISSM_MODEL_AR>{}); break;
    case VISSM_MODEL_LV: f(std::integral_constant<int, VISSM_MODEL_LV>{}); break;
    default: f(std::integral_constant<int, VISSM_MODEL_FHN>{}); break;
  }
}

// ---------------------------------------------------------------------------
// Philox4x32-10 and u01 (rng_math.hpp, shared with the host checks); Box-Muller on the 4 outputs gives
// 4 N(0,1) values.
// ---------------------------------------------------------------------------
// Box-Muller on the hardware transcendentals: r = sqrt(-2 ln u1) from v_log_f32 (log2) and
// v_sqrt_f32, the angle 2 pi u2 through v_sin_f32 / v_cos_f32, whose argument is in revolutions
// (u2 itself, in (0, 1]) -- no range reduction.  Every kernel that draws the stream uses this.
__device__ __forceinline__ void box_muller4(u4 r, float (&v)[4]) {
  constexpr float kM2Ln2 = -1.3862943611198906f;  // -2 ln 2
  const float r1 = __builtin_amdgcn_sqrtf(kM2Ln2 * __builtin_amdgcn_logf(u01(r.x)));
  const float r2 = __builtin_amdgcn_sqrtf(kM2Ln2 * __builtin_amdgcn_logf(u01(r.z)));
  const float t1 = u01(r.y), t2 = u01(r.w);
  v[0] = r1 * __builtin_amdgcn_cosf(t1);
  v[1] = r1 * __builtin_amdgcn_sinf(t1);
  v[2] = r2 * __builtin_amdgcn_cosf(t2);
  v[3] = r2 * __builtin_amdgcn_sinf(t2);
}

// Group g (four normals) of row `row` of the stream keyed (k0, k1): the forecast and the particle filters walk a row
// with this one definition, so a particle consumes the normals the forecast gives the same row.
__device__ __forceinline__ void draw4(uint32_t g, uint64_t row, uint32_t k0, uint32_t k1, float (&v)[4]) {
  const u4 c{g, 0u, static_cast<uint32_t>(row), static_cast<uint32_t>(row >> 32)};
  box_muller4(philox4x32_10(c, k0, k1), v);
}

// ---------------------------------------------------------------------------
// reductions (wave64)
// ---------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// inclusive scan over the wave's 64 lanes
__device__ __forceinline__ uint64_t wave_scan(uint64_t v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t lo = __shfl_up(static_cast<uint32_t>(v), off, 64);
    const uint32_t hi = __shfl_up(static_cast<uint32_t>(v >> 32), off, 64);
    if (lane >= off) v += (static_cast<uint64_t>(hi) << 32) | lo;
  }
  return v;
}

// Fixed-order block sum; all threads get the result.  `red` must hold blockDim/64 entries.
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  v = wave_sum(v);
  __syncthreads();
  if (lane == 0) red[wid] = v;
  __syncthreads();
  T s = 0;
  for (int i = 0; i < nw; ++i) s += red[i];
  return s;
}

__device__ __forceinline__ float elu_f(float x) { return x > 0.f ? x : expm1f(x); }
// derivative of ELU expressed through its output (TF EluGrad: y < 0 ? dy*(y+1) : dy)
__device__ __forceinline__ float elu_grad_from_out(float y) { return y < 0.f ? y + 1.f : 1.f; }
__device__ __forceinline__ float softplus_f(float x) {
  // log(1 + e^x), stable
  return x > 0.f ? x + log1pf(expf(-x)) : log1pf(expf(x));
}
__device__ __forceinline__ float sigmoid_f(float x) {
  return x >= 0.f ? 1.f / (1.f + expf(-x)) : expf(x) / (1.f + expf(x));
}

// the checks vissm_particle_filter(_adapted) and vissm_sv_filter share (particle.hip): N, the shape, K N and the
// null pointers, with the entry's name in the message; VISSM_OK or VISSM_EINVAL
int check_filter_args(const char* name, const VissmPfDesc* d, bool pointers, bool pointers_h);

constexpr float kLog2Pi = 1.8378770664093453f;
constexpr float kBnScale = 0.99950037468777f;  // 1/sqrt(1 + 1e-3)

int launch_reduce_rows(const float* slab, float* out, int64_t R, int64_t N, hipStream_t st);
// same result, two passes for few columns / many rows; uses the slab's part-head rows as scratch
int launch_reduce_rows_inplace(float* slab, float* out, int64_t R, int64_t N, hipStream_t st);
// the same sum over a slab of bf16 partials (R rows of N bf16 at `slab`), fp32 accumulation, fixed order
int launch_reduce_rows_bf16(const void* slab, float* out, int64_t R, int64_t N, hipStream_t st);

// flow epilogues shared by the flow implementations (flow_common.hip)
int launch_halo_fixup(float* du, const float* halo, int B, int L, int pL, int k, int n_chunks, int s, int CH,
                      hipStream_t st);
int launch_reduce_by_window(const float* slab, const int32_t* win, float* out, int B, int n_win, int64_t N,
                            hipStream_t st);
int launch_scatter_wgrad(const float* red, const VissmFlowGrads* g, int k, int H, int nh, int bn, hipStream_t st);

// opt-in event timing of main kernels (vissm_profile_*)
bool prof_on();
void prof_begin(int kind, hipStream_t st);
void prof_end(int kind, hipStream_t st, double bytes = 0.0);

}  // namespace vissm
