// The fused last AR flow (vissm_flow_ar_elbo_fused) and the first AR flow's backward without du: flow_v5.hip compiled
// once more, in namespace flow5f with the entry points suffixed _fz, by the Makefile with LLVM's AMDGPU
// register-pressure trackers in the scheduler (-mllvm -amdgpu-use-amdgpu-trackers=1).  That build runs the fused
// backward (bwd2_kernel<FZ = true>) 23.42 -> 22.74 ms per launch (profiles/r05/ab_sched_strategies.log) and, since the
// f16 derivative pairs, the bf16 no-du backward (bwd2_kernel<false, false>) 17.80 -> 17.26 ms
// (profiles/r07/step1_ab.txt), but the middle flows' du variant slower (20.40 -> 20.49 ms); flow_api.hip sends the
// fused entry points and the bf16 two-sample backward without du here.  Like flow_v5.o it is built without the SLP
// vectorizer (the f16-derivative products, VISSM_DERIV16).
#define VISSM_FLOW5_NS flow5f
#define VISSM_FLOW5_API(name) name##_fz
#include "flow_v5.hip"
