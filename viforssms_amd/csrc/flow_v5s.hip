// The bf16 flow kernels for three hidden layers on one window in the compiler's own MFMA register form: the shapes of
// flow_v5n.hip and 32 < k <= 64 at stride 1 (SV) -- fwd2_kernel<false, 1, 3, JB, 8, false> and bwd2n_kernel<JB, S2,
// DU>, JB <= 4 (flow5_nh3.hpp), in namespace flow5s.  Built by the Makefile with -fno-slp-vectorize as flow_v5n.hip
// but without the VGPR-form flag and the asm accumulators.  Built in the VGPR form the k > 32 kernels' gradients moved
// away from the oracle (SV k = 50 case: weight-gradient error 0.012 -> 0.51, profiles/r04/sv_vgpr_form_errs.log) while
// the k <= 24 kernels' did not; their time did not change (SV step 44.4 -> 44.2 ms), so they ship from this build.
// The k <= 24 kernels here run only under VISSM_NH3_DEFAULT_FORM=1 (flow_api.hip): tests/test_gpu_vgpr_form.py
// compares flow_v5n.hip's build of them with this one.
#define VISSM_FLOW5_NS flow5s
#include "flow5_nh3.hpp"

namespace vissm {

int flow5s_fwd(const VissmFlowDesc* d, const VissmFlowParams* w, const float* u, const float* C, const int32_t*,
               const float* theta_term, float* u_next, float* logsig, void* workspace, size_t ws_bytes,
               hipStream_t st) {
  return flow5s::nh3_fwd<4>("flow_v5s", d, w, u, C, theta_term, u_next, logsig, workspace, ws_bytes, st);
}

int flow5s_bwd(const VissmFlowDesc* d, const VissmFlowParams* w, const float* u, const float* C, const int32_t*,
               const float* theta_term, const float* du_next, const float* dlogsig, float* du, float* dC,
               float* dtheta_term, const VissmFlowGrads* gr, void* workspace, size_t ws_bytes, hipStream_t st) {
  return flow5s::nh3_bwd<4>("flow_v5s", d, w, u, C, theta_term, du_next, dlogsig, du, dC, dtheta_term, gr, workspace,
                            ws_bytes, st);
}

}  // namespace vissm
