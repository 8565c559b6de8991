// What the four translation units of the bf16 matrix-core flow (flow_v5.hip, flow_v5n.hip, flow_v5s.hip,
// flow_v5f.hip) export to flow_api.hip.  Each unit compiles the kernels of its own shapes with its own compiler flags
// (Makefile) in its own namespace; flow_api.hip alone decides which unit serves a descriptor, and a unit's launch
// function refuses a descriptor that is not its own.
#pragma once
#include "common.hpp"

namespace vissm {

// pure functions of the descriptor, the same for every unit (flow_v5.hip)
bool flow5_supports(const VissmFlowDesc* d);
size_t flow5_workspace_size(const VissmFlowDesc* d, int backward);
// which: 0 forward, 1 backward, 2 the fused last AR flow (15 outputs per 16-column tile)
void flow5_geometry(const VissmFlowDesc* d, int which, int32_t* out);
bool flow5_ar_fused_supports(const VissmFlowDesc* d);
size_t flow5_ar_fused_workspace_size(const VissmFlowDesc* d);
// whether the backward runs on the bf16 two-sample AR kernel (bwd2_kernel, single-bf16 products): without du that
// kernel ships from flow_v5f.hip
bool flow5_bwd_two_sample_bf16(const VissmFlowDesc* d);

typedef int Flow5Fwd(const VissmFlowDesc* d, const VissmFlowParams* w, const float* u, const float* C,
                     const int32_t* win, const float* theta_term, float* u_next, float* logsig, void* workspace,
                     size_t ws_bytes, hipStream_t st);
typedef int Flow5Bwd(const VissmFlowDesc* d, const VissmFlowParams* w, const float* u, const float* C,
                     const int32_t* win, const float* theta_term, const float* du_next, const float* dlogsig,
                     float* du, float* dC, float* dtheta_term, const VissmFlowGrads* gr, void* workspace,
                     size_t ws_bytes, hipStream_t st);

Flow5Fwd flow5_fwd;   // flow_v5.hip: every shape the other units do not take
Flow5Bwd flow5_bwd;
Flow5Fwd flow5n_fwd;  // flow_v5n.hip: three hidden layers, one window, k <= 24
Flow5Bwd flow5n_bwd;
Flow5Fwd flow5s_fwd;  // flow_v5s.hip: the same and 32 < k <= 64 at stride 1
Flow5Bwd flow5s_bwd;
Flow5Bwd flow5f_bwd;  // flow_v5f.hip: the bf16 two-sample AR backward without du, and the fused last AR flow
int flow5f_ar_fused(const VissmFlowDesc* d, const VissmFlowParams* w, const float* u, const float* C,
                    const int32_t* win, const float* theta_term, const float* theta, const float* obs,
                    const float* obs_bin, float obs_std, float scale, float* x, float* logsig, float* du, float* dC,
                    float* dtheta_term, const VissmFlowGrads* gr, void* workspace, size_t ws_bytes, hipStream_t st);

}  // namespace vissm
