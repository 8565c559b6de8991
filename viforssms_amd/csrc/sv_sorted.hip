// libvissm: the correlated pseudo-marginal chain of the stochastic-volatility model (vissm_sv_filter_sorted,
// vissm_sv_cpmmh; include/vissm.h; Deligiannidis, Doucet & Pitt 2018).  The chain carries the filter's random numbers
// as part of its state -- T N move normals and T resampling normals (aux_n, aux_r) -- proposes them by the
// autoregressive move u' = rho u + sqrt(1 - rho^2) eps (cpm_math.hpp) and resamples in sorted order, so that nearby u
// give nearby ancestors and the noise of ll' - ll, which is what enters the acceptance ratio, falls by an order of
// magnitude at the same N.
//
// Filter: sv_filter.hip's geometry (one block per filter, one particle per lane, N = 64 .. 1024) and its integer
// pipeline (pf_math.hpp) with two changes.  All randomness comes in through aux: no Philox here.  And each step first
// sorts the N pre-step states ascending: a bitonic network on the 32-bit keys of cpm::sort_key, one key per lane --
// the compare-exchanges of stride < 64 inside the wave by cross-lane moves with no barrier, those of stride >= 64
// through two alternating LDS arrays with one block barrier each (compile-time loops: every barrier is block-uniform).
// 21 compare-exchanges and no barrier at N = 64; 55, ten of them through LDS, at N = 1024.  The weight is a function
// of h and block-uniform data, so it is computed after the sort, on the sorted state.
//
// Chain: sv_pmmh_kernel's shell (pmmh.hip; pmmh_shell.hpp) around that step.  A chain owns two halves of aux; aux_sel
// says which belongs to its current state, the proposal is written to the other and acceptance flips aux_sel: nothing
// is copied.  A lane reads and writes entry (t, j) of aux_n only as lane j, and entry t of aux_r only as lane t mod N,
// so what an iteration wrote is read back by the thread that wrote it; the pointers are neither const nor restrict.
// The resampling normals are moved, and turned into their integers (a double erfc), by the block's lanes in parallel,
// N steps at a time, into LDS: Box-Muller and erfc stay off the serial chain.
// LDS per block = 8 N (C) + 4 N (gather) + 8 N (sort, N > 64) + 192; the chain + 4 N (U) + 256 (the factor).
#include "common.hpp"
#include "cpm_math.hpp"
#include "pf_math.hpp"
#include "pmmh_shell.hpp"
#include "svf_math.hpp"

namespace vissm {
namespace cpk {

using pmk::AdaptOut;
using pmk::Out;
using pmk::uni;

constexpr int kP = VISSM_MODEL_P(VISSM_MODEL_SV);
constexpr int sort_words(int N) { return N > 64 ? 2 * N : 1; }
constexpr int filter_lds(int N) { return 8 * N + 4 * N + 4 * sort_words(N) + 16 * (4 + 8); }

// ascending bitonic sort of one key per lane; sk [2][N] for N > 64
template <int N>
__device__ __forceinline__ uint32_t block_sort(uint32_t key, uint32_t* sk, int tid) {
  int buf = 0;
#pragma unroll
  for (int k = 2; k <= N; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      uint32_t other;
      if (j < 64) {
        other = static_cast<uint32_t>(__shfl_xor(static_cast<int>(key), j, 64));
      } else {
        // the array written two exchanges ago was read before the barrier of the last one
        sk[buf * N + tid] = key;
        __syncthreads();
        other = sk[buf * N + (tid ^ j)];
        buf ^= 1;
      }
      const bool up = (tid & k) == 0, low = (tid & j) == 0;
      key = low == up ? min(key, other) : max(key, other);
    }
  }
  return key;
}

struct Lds {
  uint64_t* Cs;
  float* xs;
  uint32_t* sk;
  float* wmax;
  uint64_t* wtot;
};

struct Step {
  float hs;    // the pre-step state this position holds after the sort
  float m;     // the maximum log-weight
  uint64_t q;  // its integer weight
  uint64_t W;  // block-uniform; 0: the filter is dead
  int anc;
};

// One step: sort, weigh, scan, resample with U, gather and move with the normal n.  h: the lane's state, in and out.
// Four barriers (A-D) beside the sort's; every thread of the block calls it.
template <int N>
__device__ __forceinline__ Step sorted_step(float& h, const sim::Par& par, const svf::Obs& ob, uint32_t U, float n,
                                            const Lds& s, int tid) {
  constexpr int NW = N / 64, LOG2N = pf::log2_of(N);
  const int lane = tid & 63, wid = tid >> 6;
  Step r;
  r.hs = cpm::key_value(block_sort<N>(cpm::sort_key(h), s.sk, tid));
  const bool ok = __builtin_isfinite(r.hs);
  const float lw = svf::state_logw(r.hs, ob);
  const float wm = wave_max(lw);
  if (lane == 0) s.wmax[wid] = wm;
  s.xs[tid] = r.hs;
  __syncthreads();  // A
  float m = s.wmax[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) m = fmaxf(m, s.wmax[w]);
  r.m = uni(m);  // the same LDS words in every thread
  r.q = pf::quantise(lw, r.m, ok);
  const uint64_t cs = wave_scan(r.q, lane);
  if (lane == 63) s.wtot[wid] = cs;
  __syncthreads();  // B
  uint64_t before = 0, W = 0;
#pragma unroll 2
  for (int w = 0; w < NW; ++w) {
    if (w < wid) before += s.wtot[w];
    W += s.wtot[w];
  }
  s.Cs[tid] = cs + before;
  r.W = uni(W);  // block-uniform: the branch below is scalar
  __syncthreads();  // C
  r.anc = tid;
  if (r.W > 0) {
    r.anc = pf::ancestor(s.Cs, N, pf::threshold(static_cast<uint32_t>(tid), U, r.W, LOG2N));
    r.anc = min(r.anc, N - 1);  // tau < W = C[N - 1]: never taken
    h = svf::move(s.xs[r.anc], par, n);
  } else {  // no live particle with a weight: the filter is dead
    h = sim::quiet_nan();
  }
  __syncthreads();  // D: the gather is over before the next step overwrites the staging arrays
  return r;
}

__device__ __forceinline__ float word_of(const float4& v, uint32_t qd) {
  return qd == 0 ? v.x : qd == 1 ? v.y : qd == 2 ? v.z : v.w;
}

// ---- the stand-alone filter ---------------------------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(N) void sv_filter_sorted_kernel(
    int T, float dt, const float* __restrict__ theta, const float* __restrict__ x_start, const float* __restrict__ obs,
    const float4* __restrict__ aux_n, const float* __restrict__ aux_r, double* __restrict__ loglik,
    float* __restrict__ ll_inc, float* __restrict__ cloud, float* __restrict__ sorted_trace,
    unsigned long long* __restrict__ q_trace, int32_t* __restrict__ anc_trace, uint32_t* __restrict__ u_trace) {
  const int tid = threadIdx.x;
  const size_t k = blockIdx.x;
  const int G = (T + 3) >> 2;

  __shared__ uint64_t Cs[N];
  __shared__ float xs[N];
  __shared__ uint32_t sk[sort_words(N)];
  __shared__ float wmax[16];
  __shared__ uint64_t wtot[16];
  const Lds lds{Cs, xs, sk, wmax, wtot};

  float th[sim::kMaxP] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < kP; ++i) th[i] = theta[k * kP + i];
  const sim::Par par = sim::prepare<VISSM_MODEL_SV>(th, dt);
  float h = x_start[k * N + tid];
  double ll = 0.0;

  // the lane's vector of group g: one group is loaded ahead
  const float4* an = aux_n + k * static_cast<size_t>(G) * N + tid;
  float4 cur = make_float4(0.f, 0.f, 0.f, 0.f), nxt = cur;
  if (G > 0) nxt = an[0];

  for (int ta = 0; ta < T; ++ta) {
    const uint32_t qd = static_cast<uint32_t>(ta) & 3u;
    if (qd == 0u) {  // uniform: the step opens a group
      cur = nxt;
      const int g = ta >> 2;
      if (g + 1 < G) nxt = an[static_cast<size_t>(g + 1) * N];
    }
    // every thread reads the same addresses: block-uniform
    const svf::Obs ob = svf::obs_prep(obs[ta], obs[static_cast<size_t>(ta) + 1], par);
    const uint32_t U = cpm::resample_u(aux_r[k * T + ta]);
    const Step r = sorted_step<N>(h, par, ob, U, word_of(cur, qd), lds, tid);
    float inc = sim::quiet_nan();
    if (r.W > 0) {
      const double li = pf::ll_increment(r.m, r.W, N);
      ll += li;
      inc = static_cast<float>(li);
    } else {
      ll = -INFINITY;
    }
    const size_t e = (k * T + ta) * N + tid;
    if (cloud) cloud[e] = h;
    if (sorted_trace) sorted_trace[e] = r.hs;
    if (q_trace) q_trace[e] = r.q;
    if (anc_trace) anc_trace[e] = r.anc;
    if (tid == 0) {
      ll_inc[k * T + ta] = inc;
      if (u_trace) u_trace[k * T + ta] = U;
    }
  }
  if (tid == 0) loglik[k] = ll;
}

// ---- the chain ----------------------------------------------------------------------------------------------------
// aux_n [C][2][G][N] float4, aux_r [C][2][T], aux_sel [C]: in and out.  adapt_end = 0: the fixed-proposal chain.
template <int N>
__global__ __launch_bounds__(N) void sv_cpmmh_kernel(uint64_t seed, uint64_t row0, int C, int n_iter, int it0, int T,
                                                     float dt, const float* __restrict__ theta_cur,
                                                     const double* __restrict__ ll_cur,
                                                     const float* __restrict__ chol_in,
                                                     const float* __restrict__ prior, const float* __restrict__ h_start,
                                                     const float* __restrict__ obs, int adapt_end, double target,
                                                     double gamma, float rho, float sigma, float4* aux_n, float* aux_r,
                                                     int32_t* aux_sel, Out o, AdaptOut a) {
  constexpr int P = kP;
  const int tid = threadIdx.x;
  const size_t c = blockIdx.x;
  const int G = (T + 3) >> 2;

  __shared__ uint64_t Cs[N];
  __shared__ float xs[N];
  __shared__ uint32_t sk[sort_words(N)];
  __shared__ uint32_t us[N];  // the resampling integers of N steps
  __shared__ float wmax[16];
  __shared__ uint64_t wtot[16];
  // the update's doubles, then the factor
  __shared__ double Ws[pmk::adapt_lds_doubles(P)];
  float* const Ls = reinterpret_cast<float*>(Ws + mh::adapt_work(P));
  const Lds lds{Cs, xs, sk, wmax, wtot};

  // the chain's state and the launch's constants: block-uniform
  float th[mh::kMaxP] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < P; ++i) th[i] = theta_cur[c * P + i];
  const float h0 = h_start[0];
  double ll = ll_cur[c];
  double lp = uni(mh::log_prior(th, prior, P));
  int sel = __builtin_amdgcn_readfirstlane(aux_sel[c]) & 1;  // which half goes with (theta, ll)
  const uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
  pmk::load_factor<P>(Ls, chol_in, c, tid);
  const bool traced = a.xi_trace || a.alpha_trace || a.eta_trace || a.chol_trace;
  const size_t half_n = static_cast<size_t>(G) * N, half_r = static_cast<size_t>(T);

  for (int it = 0; it < n_iter; ++it) {
    const uint64_t frow = mh::row_of(row0, static_cast<uint64_t>(it0) + it, C, c, N);
    // block-uniform: the absolute iteration is below adapt_end
    const bool adapting = static_cast<int64_t>(it0) + it < adapt_end;
    const float* pr = prior;
    asm volatile("" : "+s"(pr));  // read again in every iteration, as in pmmh_kernel

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
      mh::propose(th, Ls, xi, P, thp);
#pragma unroll
      for (int i = 0; i < P; ++i) thp[i] = uni(thp[i]);
    }
    // every wave has read the factor before thread 0 rewrites it (T = 0: the filter loop passes no barrier)
    if (adapting) __syncthreads();

    // the sorted filter at theta' over steps 0 .. T - 1, on the proposed aux, which it writes to the other half
    const sim::Par par = sim::prepare<VISSM_MODEL_SV>(thp, dt);
    float h = h0;
    double llp = 0.0;
    const uint64_t row = frow + static_cast<uint64_t>(tid);
    const float4* an_cur = aux_n + (c * 2 + sel) * half_n + tid;
    float4* an_new = aux_n + (c * 2 + (sel ^ 1)) * half_n + tid;
    const float* ar_cur = aux_r + (c * 2 + sel) * half_r;
    float* ar_new = aux_r + (c * 2 + (sel ^ 1)) * half_r;
    float eps[4];  // the normals and the carried values of the next group
    float4 cur = make_float4(0.f, 0.f, 0.f, 0.f), un = cur;
    draw4(0u, row, k0, k1, eps);
    if (G > 0) un = an_cur[0];

    for (int ta = 0; ta < T; ++ta) {
      if ((ta & (N - 1)) == 0) {  // uniform: the resampling normals of steps ta .. ta + N - 1, one per lane
        const int t = ta + tid;
        if (t < T) {
          const u4 ctr{static_cast<uint32_t>(t), 1u, static_cast<uint32_t>(frow), static_cast<uint32_t>(frow >> 32)};
          float v[4];
          box_muller4(philox4x32_10(ctr, k0, k1), v);
          const float urp = cpm::cn(ar_cur[t], v[0], rho, sigma);
          ar_new[t] = urp;
          us[tid] = cpm::resample_u(urp);
        }
        __syncthreads();  // (the last read of us was before barrier D of the step before)
      }
      const uint32_t qd = static_cast<uint32_t>(ta) & 3u;
      if (qd == 0u) {  // uniform: the step opens a group; its four moved normals, then the next group's inputs
        const int g = ta >> 2;
        cur.x = cpm::cn(un.x, eps[0], rho, sigma);
        cur.y = ta + 1 < T ? cpm::cn(un.y, eps[1], rho, sigma) : 0.f;
        cur.z = ta + 2 < T ? cpm::cn(un.z, eps[2], rho, sigma) : 0.f;
        cur.w = ta + 3 < T ? cpm::cn(un.w, eps[3], rho, sigma) : 0.f;
        an_new[static_cast<size_t>(g) * N] = cur;
        draw4(static_cast<uint32_t>(g) + 1u, row, k0, k1, eps);
        if (g + 1 < G) un = an_cur[static_cast<size_t>(g + 1) * N];
      }
      // every thread reads the same addresses: block-uniform
      const svf::Obs ob = svf::obs_prep(obs[ta], obs[static_cast<size_t>(ta) + 1], par);
      const uint32_t U = us[ta & (N - 1)];
      const Step r = sorted_step<N>(h, par, ob, U, word_of(cur, qd), lds, tid);
      if (r.W == 0) {  // the proposal is dead; the rest of its half stays unwritten and is never selected
        llp = -INFINITY;
        break;
      }
      llp = uni(llp + pf::ll_increment(r.m, r.W, N));
    }

    // the decision
    const double lpp = mh::log_prior(thp, pr, P);
    const double logu = mh::log_uniform(mh::words(2u, frow, seed).x);
    // the acceptance probability, from the state before the decision
    double al = 0.0;
    if (adapting || traced) al = uni(mh::accept_prob(llp, ll, lpp, lp));
    const bool acc = __builtin_amdgcn_readfirstlane(mh::accept(logu, llp, ll, lpp, lp) ? 1 : 0) != 0;
    if (acc) {
#pragma unroll
      for (int i = 0; i < P; ++i) th[i] = thp[i];
      ll = uni(llp);
      lp = uni(lpp);
      sel ^= 1;
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
        pmk::adapt_step<P>(Ls, Ws, frow, seed, adapting, static_cast<int64_t>(it0) + it, al, target, gamma, a, e);
    }
    // thread 0's factor is in LDS before the next iteration's proposal reads it
    if (adapting) __syncthreads();
  }
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < P; ++i) o.theta_end[c * P + i] = th[i];
    o.ll_end[c] = ll;
    aux_sel[c] = sel;
#pragma unroll
    for (int i = 0; i < P * P; ++i) a.chol_end[c * (P * P) + i] = Ls[i];
  }
}

}  // namespace cpk
}  // namespace vissm

using namespace vissm;
using namespace vissm::cpk;

extern "C" int32_t vissm_sv_filter_sorted_lds_bytes(int32_t N) { return pf::valid_n(N) ? filter_lds(N) : 0; }

extern "C" int vissm_sv_filter_sorted(const VissmPfDesc* d, const float* theta, const float* x_start, const float* obs,
                                      const float* aux_n, const float* aux_r, double* loglik, float* ll_inc,
                                      float* cloud, float* sorted_trace, uint64_t* q_trace, int32_t* anc_trace,
                                      uint32_t* u_trace, void* stream) {
  // host arithmetic only, before any GPU call
  VISSM_CHECK_ARG(d, "sv_filter_sorted: null descriptor");
  VISSM_CHECK_ARG(d->model == VISSM_MODEL_SV, "sv_filter_sorted: model %d is not SV", d->model);
  if (const int rc = check_filter_args("sv_filter_sorted", d, theta && x_start && loglik,
                                       obs && ll_inc && aux_n && aux_r))
    return rc;
  VISSM_CHECK_ARG(d->t0 == 0 && d->H == d->T_total,
                  "sv_filter_sorted: t0=%d H=%d: the whole series only (t0 = 0, H = T_total = %d)", d->t0, d->H,
                  d->T_total);
  VISSM_CHECK_ARG(d->T_total < 2147483647, "sv_filter_sorted: T_total=%d", d->T_total);
  VISSM_CHECK_ARG(reinterpret_cast<uintptr_t>(aux_n) % 16 == 0, "sv_filter_sorted: aux_n must be 16-byte aligned");
  // (a NaN fails the first comparison, an infinity the second)
  VISSM_CHECK_ARG(d->dt > 0.f && d->dt <= 3.4028234e38f, "sv_filter_sorted: dt must be positive and finite, got %g",
                  static_cast<double>(d->dt));
  if (d->K == 0) return VISSM_OK;
  dispatch_n(d->N, [&](auto n) {
    hipLaunchKernelGGL((sv_filter_sorted_kernel<decltype(n)::value>), dim3(d->K), dim3(d->N), 0, as_stream(stream),
                       d->T_total, d->dt, theta, x_start, obs, reinterpret_cast<const float4*>(aux_n), aux_r, loglik,
                       ll_inc, cloud, sorted_trace, reinterpret_cast<unsigned long long*>(q_trace), anc_trace, u_trace);
  });
  VISSM_CHECK_LAUNCH("sv_filter_sorted");
  return VISSM_OK;
}

extern "C" int32_t vissm_sv_cpmmh_lds_bytes(int32_t N) {
  return pf::valid_n(N) ? filter_lds(N) + 4 * N + 8 * pmk::adapt_lds_doubles(kP) : 0;
}

extern "C" int vissm_sv_cpmmh(const VissmPmmhDesc* d, uint64_t seed, uint64_t row0, const float* theta_cur,
                              const double* ll_cur, const float* chol_in, const float* prior, const float* h_start,
                              const float* obs, int32_t adapt_end, double target_accept, double gamma, float rho,
                              float* aux_n, float* aux_r, int32_t* aux_sel, float* theta_chain, double* ll_chain,
                              int32_t* accept, float* theta_end, double* ll_end, float* chol_end, float* theta_prop,
                              double* ll_prop, double* logu, float* xi_trace, double* alpha_trace, double* eta_trace,
                              float* chol_trace, void* stream) {
  // host arithmetic only, before any GPU call
  const char* name = "sv_cpmmh";
  VISSM_CHECK_ARG(d, "%s: null descriptor", name);
  VISSM_CHECK_ARG(d->model == VISSM_MODEL_SV, "%s: model %d is not SV (the other models have no sorted filter)", name,
                  d->model);
  if (const int rc = pmk::check_chain_args(name, d, theta_cur && ll_cur && prior && h_start && theta_end && ll_end,
                                           theta_chain && ll_chain && accept, obs != nullptr))
    return rc;
  if (const int rc = pmk::check_adapt_args(name, adapt_end, target_accept, gamma, chol_in, chol_end)) return rc;
  // (the series holds T_total + 1 values and step ta reads y[ta + 1])
  VISSM_CHECK_ARG(d->T_total >= 0 && d->T_total < 2147483647, "%s: T_total=%d", name, d->T_total);
  // (a NaN fails the first comparison, an infinity the second)
  VISSM_CHECK_ARG(d->dt > 0.f && d->dt <= 3.4028234e38f, "%s: dt must be positive and finite, got %g", name,
                  static_cast<double>(d->dt));
  VISSM_CHECK_ARG(cpm::valid_rho(rho), "%s: rho=%g outside [0, 1)", name, static_cast<double>(rho));
  VISSM_CHECK_ARG(aux_n && aux_r && aux_sel, "%s: null pointer (aux_n, aux_r, aux_sel)", name);
  VISSM_CHECK_ARG(reinterpret_cast<uintptr_t>(aux_n) % 16 == 0, "%s: aux_n must be 16-byte aligned", name);
  const Out o{theta_chain, ll_chain, accept, theta_end, ll_end, theta_prop, ll_prop, logu};
  const AdaptOut a{chol_end, xi_trace, alpha_trace, eta_trace, chol_trace};
  const float sigma = cpm::sigma_of(rho);
  dispatch_n(d->N, [&](auto n) {
    hipLaunchKernelGGL((sv_cpmmh_kernel<decltype(n)::value>), dim3(d->C), dim3(d->N), 0, as_stream(stream), seed, row0,
                       d->C, d->n_iter, d->it0, d->T_total, d->dt, theta_cur, ll_cur, chol_in, prior, h_start, obs,
                       adapt_end, target_accept, gamma, rho, sigma, reinterpret_cast<float4*>(aux_n), aux_r, aux_sel, o,
                       a);
  });
  VISSM_CHECK_LAUNCH(name);
  return VISSM_OK;
}
