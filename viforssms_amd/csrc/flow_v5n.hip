// The bf16 flow kernels for three hidden layers on one window at k <= 24 (LV / FHN heads): fwd2_kernel<false, 1, 3,
// JB, 8, false> and bwd2n_kernel<JB, S2, DU>, JB <= 2 (flow5_nh3.hpp), in namespace flow5n.  The Makefile builds this
// unit with -fno-slp-vectorize: without the SLP vectorizer the element-wise work beside the matrix-core chains
// stays in scalar VALU instructions instead of v_pk_fma_f32 / v_pk_mul_f32, which cost more than two scalar ones
// between MFMAs (MI355X_MICROARCH.md, filler prices): LV-cfg backward 18.1 -> 16.8 ms per launch (A/B,
// profiles/r03/ab_misc_r03.log), FHN 3.7 -> 3.5 ms, SV 7.2 -> 6.7 ms; the one-hidden-layer AR kernels (+0.3 ms per
// launch) and the one-sample three-layer backward (SV's k = 50: 10.3 -> 10.8 ms) measured slower that way and keep
// the vectorizer.
// Also built with -mllvm -amdgpu-mfma-vgpr-form=1: with 512 registers per wave the compiler otherwise writes the
// chain's MFMA results (the recompute, dX, dcon) into AGPRs and copies every element back for the element-wise work
// (508 v_accvgpr_read + 215 v_accvgpr_mov of 2021 VALU instructions per pair unit at LV); in the VGPR form, with the
// item-lifetime dW / dW_eps / dW_head accumulators pinned to the AGPRs by inline asm (mfma32_a*, flow_v5.hip:
// VISSM_BWD2N_AACC), the pair unit issues 1535-1685 VALU instructions: LV backward 16.6 -> 14.6 ms per launch, FHN
// 3.45 -> 3.06 ms (profiles/r04/ab_families_vgpr_form.log).
#define VISSM_BWD2N_AACC 1
#define VISSM_FLOW5_NS flow5n
#include "flow5_nh3.hpp"

namespace vissm {

int flow5n_fwd(const VissmFlowDesc* d, const VissmFlowParams* w, const float* u, const float* C, const int32_t*,
               const float* theta_term, float* u_next, float* logsig, void* workspace, size_t ws_bytes,
               hipStream_t st) {
  return flow5n::nh3_fwd<2>("flow_v5n", d, w, u, C, theta_term, u_next, logsig, workspace, ws_bytes, st);
}

int flow5n_bwd(const VissmFlowDesc* d, const VissmFlowParams* w, const float* u, const float* C, const int32_t*,
               const float* theta_term, const float* du_next, const float* dlogsig, float* du, float* dC,
               float* dtheta_term, const VissmFlowGrads* gr, void* workspace, size_t ws_bytes, hipStream_t st) {
  return flow5n::nh3_bwd<2>("flow_v5n", d, w, u, C, theta_term, du_next, dlogsig, du, dC, dtheta_term, gr, workspace,
                            ws_bytes, st);
}

}  // namespace vissm
