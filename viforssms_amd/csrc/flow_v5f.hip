// The fused last AR flow (vissm_flow_ar_elbo_fused) and the first AR flow's backward without du, in namespace flow5f,
// built by the Makefile with LLVM's AMDGPU register-pressure trackers in the scheduler
// (-mllvm -amdgpu-use-amdgpu-trackers=1).  That build runs the fused backward (bwd2_kernel<FZ = true>) 23.42 ->
// 22.74 ms per launch (profiles/r05/ab_sched_strategies.log) and, since the f16 derivative pairs, the bf16 no-du
// backward (bwd2_kernel<false, false>) 17.80 -> 17.26 ms, no scratch in either build, the same arithmetic
// (profiles/r07/step1_ab.txt), but the middle flows' du variant slower (20.40 -> 20.49 ms): that one stays in
// flow_v5.hip.  Like flow_v5.o it is built without the SLP vectorizer (the f16-derivative products, VISSM_DERIV16).
// Kernels (flow5f_kernel_order below): bwd2_kernel<true, true, TF, NPR, SB> for (NPR, SB) = (1, false), (2, false), (2, true) and
// bwd_kernel<1, 1, JB <= 2, NP = 1 | 3, true> (the fused flow); bwd2_kernel<false, false, TF, 1, false> (no du).
#define VISSM_FLOW5_NS flow5f
#include "flow_v5.hip"

namespace vissm {
using namespace flow5f;

// The unit's kernels, in the order in which they are instantiated.  The order is part of the build: hipcc inlines the
// shared __forceinline__ helpers (mm, split8, put_image, tr_read, ...) in the order in which they first entered the
// module, and the one-sample bwd_kernel's instruction stream follows that order (its registers, scratch and LDS do
// not).  This is the order of the build in which every kernel was measured, when each unit still instantiated all
// families (scripts/compare_kernel_asm.py against that build: every stream identical,
// profiles/r08/asm_compare.txt).  Entries marked "order only" are never launched from this unit: they are the
// fewest kernels of other routes that bring the shared helpers in in that order
// (profiles/r08/asm_compare_notes.txt).  A kernel added to the unit goes at the end.
const void* flow5f_kernel_order(int i) {
  static const void* const k[] = {
      (const void*)fwd_kernel<1, 1, 2, 3>, (const void*)fwd_kernel<1, 1, 2, 1>,  // order only (flow_v5 launches them)
      (const void*)fwd_kernel<3, 1, 1, 1>,                                        // order only
      (const void*)bwd2n_kernel<1, true, true>,  // order only (flow_v5n / flow_v5s launch it)
      (const void*)bwd2_kernel<false, false, true, 1, false>, (const void*)bwd2_kernel<false, false, false, 1, false>,
      (const void*)bwd2_kernel<true, true, true, 2, true>, (const void*)bwd2_kernel<true, true, false, 2, true>,
      (const void*)bwd2_kernel<true, true, true, 2, false>, (const void*)bwd2_kernel<true, true, false, 2, false>,
      (const void*)bwd2_kernel<true, true, true, 1, false>, (const void*)bwd2_kernel<true, true, false, 1, false>,
      (const void*)bwd_kernel<1, 1, 1, 3, true, true>, (const void*)bwd_kernel<1, 1, 2, 3, true, true>,
      (const void*)bwd_kernel<1, 1, 1, 1, true, true>, (const void*)bwd_kernel<1, 1, 2, 1, true, true>,
  };
  return k[i];
}

// the bf16 two-sample AR backward without du (flow5_bwd_two_sample_bf16): the workspace layout is flow_v5.hip's
int flow5f_bwd(const VissmFlowDesc* d, const VissmFlowParams* w, const float* u, const float* C, const int32_t* win,
               const float* theta_term, const float* du_next, const float* dlogsig, float* du, float* dC,
               float* dtheta_term, const VissmFlowGrads* gr, void* workspace, size_t ws_bytes, hipStream_t st) {
  Launch L;
  L.g = geom(d, true);
  VISSM_CHECK_ARG(!du && np_of(d) == 1 && !bwd2n_ok(d, L.g) && bwd2_ok(d, L.g),
                  "flow_v5f: runs only the bf16 two-sample AR backward without du");
  const bool fold = fold_ok(d, w);
  int rc = prologue(&L, d, w, C, theta_term, workspace, ws_bytes, 1, fold, false, "flow_bwd", st);
  if (rc) return rc;
  prof_begin(VISSM_PROF_FLOW_BWD, st);
  prof_begin(VISSM_PROF_FLOW_BWD_NODU, st);
  if (fold) launch_bwd2<false, false, true, 1, false>(L, u, du_next, dlogsig, du, FzArgs{}, st);
  else launch_bwd2<false, false, false, 1, false>(L, u, du_next, dlogsig, du, FzArgs{}, st);
  VISSM_CHECK_LAUNCH("flow5_bwd");
  prof_end(VISSM_PROF_FLOW_BWD_NODU, st);
  prof_end(VISSM_PROF_FLOW_BWD, st);
  return bwd_epilogue(L, d, w, win, du, dC, dtheta_term, nullptr, gr, st);
}

// ---- the last AR(1) flow fused with its ELBO terms (vissm_flow_ar_elbo_fused) ----
template <int JB, int NP>
static void launch_bwd_fz(const Launch& L, const float* u, const int32_t* wn, float* du, const FzArgs& fz,
                          hipStream_t st) {
  hipLaunchKernelGGL((bwd_kernel<1, 1, JB, NP, true>), dim3(L.g.blocks), dim3(NT), 0, st, L.a, u, L.ws.Cp, wn, L.ws.thp,
                     static_cast<const float*>(nullptr), static_cast<const float*>(nullptr), L.ws.img, L.ws.cst, du,
                     L.ws.dC_slab, L.ws.dth_slab, L.ws.dW_slab, L.ws.halo, fz);
}

int flow5f_ar_fused(const VissmFlowDesc* d, const VissmFlowParams* w, const float* u, const float* C,
                    const int32_t* win, const float* theta_term, const float* theta, const float* obs,
                    const float* obs_bin, float obs_std, float scale, float* x, float* logsig, float* du, float* dC,
                    float* dtheta_term, const VissmFlowGrads* gr, void* workspace, size_t ws_bytes, hipStream_t st) {
  VISSM_CHECK_ARG(flow5_ar_fused_supports(d), "flow_v5f: the descriptor has no fused AR(1) last flow");
  VISSM_CHECK_ARG(du && logsig, "flow_v5f: the fused flow writes du and log sigma (null pointer)");
  Launch L;
  L.g = geom(d, true, P - 1);
  // bf16x2: split-weight recompute and backward chain; bf16x2_bf16: split-weight recompute, bf16 backward products
  const bool x2 = d->precision == VISSM_PREC_BF16X2 || d->precision == VISSM_PREC_BF16X2_BF16;
  const bool sb = d->precision == VISSM_PREC_BF16X2;
  // bf16x2 has only the two-sample kernel: it must meet that kernel's geometry (bwd2_ok minus the precision test)
  VISSM_CHECK_ARG(!x2 || (L.g.S == S && d->n_win == 1 && d->k <= KP2),
                  "flow_ar_elbo_fused: bf16x2 needs the two-sample kernel's geometry (one window, k <= %d)", KP2);
  const bool b2 = x2 || bwd2_ok(d, L.g), fold = b2 && fold_ok(d, w);
  int rc = prologue(&L, d, w, C, theta_term, workspace, ws_bytes, 2, fold, x2 && lofold_ok(d), "flow_ar_elbo_fused", st);
  if (rc) return rc;
  FzArgs fz;
  fz.theta = theta;
  fz.obs = obs;
  fz.bin = obs_bin;
  fz.x = x;
  fz.lsl = L.ws.zsl;
  fz.scale = scale;
  fz.iosd = 1.f / obs_std;
  fz.M = d->L - d->k - 1;
  prof_begin(VISSM_PROF_FLOW_BWD, st);
  prof_begin(VISSM_PROF_FLOW_FUSED, st);
  if (b2) {
    if (sb) {
      if (fold) launch_bwd2<true, true, true, 2, true>(L, u, nullptr, nullptr, du, fz, st);
      else launch_bwd2<true, true, false, 2, true>(L, u, nullptr, nullptr, du, fz, st);
    } else if (x2) {
      if (fold) launch_bwd2<true, true, true, 2, false>(L, u, nullptr, nullptr, du, fz, st);
      else launch_bwd2<true, true, false, 2, false>(L, u, nullptr, nullptr, du, fz, st);
    } else {
      if (fold) launch_bwd2<true, true, true, 1, false>(L, u, nullptr, nullptr, du, fz, st);
      else launch_bwd2<true, true, false, 1, false>(L, u, nullptr, nullptr, du, fz, st);
    }
  } else {
    const int32_t* wn = d->n_win > 1 ? win : nullptr;
    const int jb = jb_of(d->k);
    if (np_of(d) == 3) {
      if (jb == 1) launch_bwd_fz<1, 3>(L, u, wn, du, fz, st);
      else launch_bwd_fz<2, 3>(L, u, wn, du, fz, st);
    } else {
      if (jb == 1) launch_bwd_fz<1, 1>(L, u, wn, du, fz, st);
      else launch_bwd_fz<2, 1>(L, u, wn, du, fz, st);
    }
  }
  VISSM_CHECK_LAUNCH("flow5_fused");
  prof_end(VISSM_PROF_FLOW_FUSED, st);
  prof_end(VISSM_PROF_FLOW_BWD, st);
  return bwd_epilogue(L, d, w, win, du, dC, dtheta_term, logsig, gr, st);
}

}  // namespace vissm
