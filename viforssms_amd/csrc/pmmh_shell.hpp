// What the Metropolis-Hastings kernels share around their filters (pmmh.hip: pmmh_kernel, sv_pmmh_kernel; sv_sorted.hip:
// sv_cpmmh_kernel): block-uniform values in scalar registers, the chains' output pointers, the adaptive chains' factor in
// LDS and its update after the decision, and the host checks of the entries.  Device code: included by .hip units only.
#pragma once
#include "common.hpp"
#include "mh_math.hpp"

namespace vissm {
namespace pmk {

// A block-uniform value the vector ALU computed, moved to a scalar register: the chain's state and the proposal live
// across the whole filter loop, where the 1024-lane block has no vector registers to spare for them.
__device__ __forceinline__ float uni(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
__device__ __forceinline__ uint64_t uni(uint64_t b) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(b));
  const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(b >> 32));
  return (static_cast<uint64_t>(hi) << 32) | lo;
}
__device__ __forceinline__ double uni(double v) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(b));
  const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(b >> 32));
  return __builtin_bit_cast(double, (static_cast<uint64_t>(hi) << 32) | lo);
}

struct Out {
  float* theta_chain;
  double* ll_chain;
  int32_t* accept;
  float* theta_end;
  double* ll_end;
  float* theta_prop;
  double* ll_prop;
  double* logu;
};

// ---- the adaptive chains (vissm_pmmh_adaptive, vissm_sv_pmmh_adaptive) ---------------------------------------------
// pmmh_kernel and sv_pmmh_kernel (pmmh.hip) with ADAPT = true: a factor per chain that follows mh::adapt (mh_math.hpp:
// robust adaptive Metropolis) while the absolute iteration it0 + it is below adapt_end, and is frozen after: from then
// on the chain is bit for bit the fixed-proposal chain with that factor.  The two variants are one __global__ template
// with a bool flag, the additions under if constexpr (ADAPT) or ADAPT && ...: the compiler sees each instantiation
// as the kernel it was when the two were written out, and every one of the 40 keeps its instruction stream and its
// registers (the fixed ones read their arguments from a longer segment; profiles/r26/compare_kernel_asm.txt).  A
// __device__ body called from thin kernels does not: inlined, it is scheduled otherwise.
//
// The factor lives in LDS (4 P P bytes): the proposal reads it as a broadcast, thread 0 rewrites it after the decision,
// working on a double copy that sits in LDS too (8 (P P + 2 P) bytes with v and xi; mh::adapt_work): with the copy in
// registers the 1024-lane blocks spilled.
// It is not kept in global memory and read back through the const __restrict__ pointer: uniform reads of such a
// pointer go through the scalar data cache, which does not see the vector stores of the same kernel.  Two block-uniform
// barriers per adapting iteration order the accesses: one after the proposal (every wave has read the factor; the
// filter loop passes no barrier when no step is observed), one after the update.  Nothing of the update is live over
// the filter loop: the normals are drawn again from their two Philox blocks (the same function, the same bits) and the
// update's doubles live in thread 0's scope after the decision.
// LDS per block = the twin's + 8 (P P + 2 P) + 8 ceil(P P / 2): one array of doubles, the factor's floats at its end.
constexpr int adapt_lds_doubles(int P) { return mh::adapt_work(P) + (P * P + 1) / 2; }
struct AdaptOut {
  float* chol_end;
  float* xi_trace;
  double* alpha_trace;
  double* eta_trace;
  float* chol_trace;
};

// chain c's lower factor into LDS, the strict upper part 0
template <int P>
__device__ __forceinline__ void load_factor(float* Ls, const float* __restrict__ chol_in, size_t c, int tid) {
  if (tid < P * P) Ls[tid] = tid % P <= tid / P ? chol_in[c * (P * P) + tid] : 0.f;
  __syncthreads();
}

// thread 0, after the decision of entry e = c n_iter + it: the factor's update and the traces
template <int P>
__device__ __forceinline__ void adapt_step(float* Ls, double* Ws, uint64_t frow, uint64_t seed, bool adapting, int64_t i, double al,
                                           double target, double gamma, const AdaptOut& a, size_t e) {
  asm volatile("" : "+s"(frow));  // drawn again, not carried over the filter loop
  float xi[8], v[4];
  box_muller4(mh::words(0u, frow, seed), v);
#pragma unroll
  for (int j = 0; j < 4; ++j) xi[j] = v[j];
  box_muller4(mh::words(1u, frow, seed), v);
#pragma unroll
  for (int j = 0; j < 4; ++j) xi[4 + j] = v[j];
  double eta = 0.0;
  if (adapting) {
    eta = mh::adapt_eta(P, i, gamma);
    mh::adapt(Ls, xi, al, eta, target, P, Ws);
  }
  if (a.xi_trace) {
#pragma unroll
    for (int j = 0; j < 8; ++j) a.xi_trace[e * 8 + j] = xi[j];
  }
  if (a.alpha_trace) a.alpha_trace[e] = al;
  if (a.eta_trace) a.eta_trace[e] = eta;
  if (a.chol_trace) {
#pragma unroll
    for (int j = 0; j < P * P; ++j) a.chol_trace[e * (P * P) + j] = Ls[j];
  }
}

// the checks the chain entries share, with the entry's name in the message (pmmh.hip)
int check_chain_args(const char* name, const VissmPmmhDesc* d, bool pointers, bool pointers_iter, bool pointers_t);
// the checks the adaptive entries add (pmmh.hip)
int check_adapt_args(const char* name, int32_t adapt_end, double target_accept, double gamma, const void* chol_in,
                     const void* chol_end);

}  // namespace pmk
}  // namespace vissm
