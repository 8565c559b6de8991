// Host side of the two translation units that run the three-hidden-layer shapes on one window (LV / SV / FHN heads):
// flow_v5n.hip (k <= 24: JB_MAX = 2) and flow_v5s.hip (the same and 32 < k <= 64 at stride 1: JB_MAX = 4).  The
// forward is fwd2_kernel<false, 1, 3, JB, 8, false>, the backward bwd2n_kernel<JB, S2, DU>, JB = ceil(k / 16) <= JB_MAX;
// a unit instantiates nothing else.
#pragma once
#include "flow_v5.hip"

namespace vissm {
namespace VISSM_FLOW5_NS {

// the unit's own shapes: those of bwd2n_kernel up to its JB_MAX.  The forward asks the same question: for bf16, three
// hidden layers and one window, fwd2_ok holds wherever bwd2n_ok does (k <= 24, or 32 < k <= 64 at stride 1), and
// those are the only shapes use_nh3 / use_nh3s (flow_api.hip) send here
template <int JB_MAX>
static int nh3_check(const char* unit, const VissmFlowDesc* d, const Geom& g) {
  VISSM_CHECK_ARG(bwd2n_ok(d, g) && jb_of(d->k) <= JB_MAX, "%s: not a shape of this unit (bf16, three hidden layers, "
                  "one window, k <= 24%s; n_hidden=%d n_win=%d k=%d)", unit,
                  JB_MAX > 2 ? " or 32 < k <= 64 at stride 1" : "", d->n_hidden, d->n_win, d->k);
  return VISSM_OK;
}

template <int JB_MAX>
static int nh3_fwd(const char* unit, const VissmFlowDesc* d, const VissmFlowParams* w, const float* u, const float* C,
                   const float* theta_term, float* u_next, float* logsig, void* workspace, size_t ws_bytes,
                   hipStream_t st) {
  Launch L;
  L.g = geom(d, false);
  int rc = nh3_check<JB_MAX>(unit, d, L.g);
  if (rc) return rc;
  rc = prologue(&L, d, w, C, theta_term, workspace, ws_bytes, 0, false, false, "flow_fwd", st);
  if (rc) return rc;
  prof_begin(VISSM_PROF_FLOW_FWD, st);
  const int jb = jb_of(d->k);
  if (jb == 1) launch_fwd2<false, 1, 3, 1, false>(L, u, u_next, st);
  else if (jb == 2) launch_fwd2<false, 1, 3, 2, false>(L, u, u_next, st);
  else if constexpr (JB_MAX > 2) {
    if (jb == 3) launch_fwd2<false, 1, 3, 3, false>(L, u, u_next, st);
    else launch_fwd2<false, 1, 3, 4, false>(L, u, u_next, st);
  } else {
    VISSM_CHECK_ARG(false, "%s: no forward kernel for k=%d", unit, d->k);
  }
  return fwd_epilogue(L, d, logsig, st);
}

template <int JB, bool S2>
static void launch_bwd2n_du(const Launch& L, const float* u, const float* du_next, const float* dlogsig, float* du,
                            hipStream_t st) {
  if (du) launch_bwd2n<JB, S2, true>(L, u, du_next, dlogsig, du, st);
  else launch_bwd2n<JB, S2, false>(L, u, du_next, dlogsig, du, st);
}

template <int JB_MAX>
static int nh3_bwd(const char* unit, const VissmFlowDesc* d, const VissmFlowParams* w, const float* u, const float* C,
                   const float* theta_term, const float* du_next, const float* dlogsig, float* du, float* dC,
                   float* dtheta_term, const VissmFlowGrads* gr, void* workspace, size_t ws_bytes, hipStream_t st) {
  Launch L;
  L.g = geom(d, true);
  int rc = nh3_check<JB_MAX>(unit, d, L.g);
  if (rc) return rc;
  rc = prologue(&L, d, w, C, theta_term, workspace, ws_bytes, 1, false, false, "flow_bwd", st);
  if (rc) return rc;
  const int pvar = du ? VISSM_PROF_FLOW_BWD_DU : VISSM_PROF_FLOW_BWD_NODU;
  prof_begin(VISSM_PROF_FLOW_BWD, st);
  prof_begin(pvar, st);
  const int jb = jb_of(d->k);
  if (d->stride2) {  // k <= 24
    if (jb == 1) launch_bwd2n_du<1, true>(L, u, du_next, dlogsig, du, st);
    else launch_bwd2n_du<2, true>(L, u, du_next, dlogsig, du, st);
  } else if (jb == 1) launch_bwd2n_du<1, false>(L, u, du_next, dlogsig, du, st);
  else if (jb == 2) launch_bwd2n_du<2, false>(L, u, du_next, dlogsig, du, st);
  else if constexpr (JB_MAX > 2) {
    if (jb == 3) launch_bwd2n_du<3, false>(L, u, du_next, dlogsig, du, st);
    else launch_bwd2n_du<4, false>(L, u, du_next, dlogsig, du, st);
  } else {
    VISSM_CHECK_ARG(false, "%s: no backward kernel for k=%d", unit, d->k);
  }
  VISSM_CHECK_LAUNCH("flow5_bwd");
  prof_end(pvar, st);
  prof_end(VISSM_PROF_FLOW_BWD, st);
  return bwd_epilogue(L, d, w, nullptr, du, dC, dtheta_term, nullptr, gr, st);
}

}  // namespace VISSM_FLOW5_NS
}  // namespace vissm
