"""posterior_summary over data-parallel ranks: 2 ranks share cuda:0 over gloo (spawned as in tests/test_gpu_dist.py;
each rank a fresh child process).  The Philox rows are keyed by the global sample index, so the two ranks' halves
are together the sample set of one process holding the full batch; the select's only cross-rank quantity is an
integer histogram (SUM all-reduce), so the quantiles are bitwise equal on both ranks and equal to the single
process's.  The means' double sums are reduced in another order: within the moments' bound."""
import numpy as np
import pytest

from tests.dist_util import attach, run_ranks

pytestmark = pytest.mark.gpu

P = 16
SHAPE, T = (P, 30, 5, 2, 20, 3, 4), 60     # AR: (B, M, k, n_flows, H, n_layers, fw), two windows
PROBS = (0.0, 0.025, 0.5, 0.975, 1.0)       # with the extremes: max|x| per column bounds the means' error
KEYS = ("paths/mean", "paths/sd", "paths/quantiles", "paths/n_valid", "theta/mean", "theta/sd", "theta/quantiles",
        "theta/n_valid")


def _model():
    from tests.parity_util import build_model
    return build_model("ar", *SHAPE, "cuda:0", T=T, precision=0, seed=3)


def _worker(rank, world):
    model = attach(_model(), rank, world, P)
    res = model.posterior_summary(PROBS)
    return {k: res[k] for k in KEYS}


def test_two_rank_summary_equals_full_batch():
    res = run_ranks(_worker)      # both children have exited (exit codes checked) before this process touches the GPU
    full = _model().posterior_summary(PROBS)
    r0, r1 = res[0], res[1]
    for k in KEYS:
        assert np.array_equal(r0[k], r1[k], equal_nan=True), k          # replicated result: bitwise on both ranks
    for k in ("paths/quantiles", "theta/quantiles", "paths/n_valid", "theta/n_valid"):
        assert np.array_equal(r0[k], full[k]), k                        # exact over the union of the ranks' samples
    assert full["paths/quantiles"].shape == (5, 1, T) and np.all(full["paths/n_valid"] == P)
    # means: the two halves' sums added vs one pass, each within 2 B 2^-53 sum|x| of the exact sum, so the means
    # differ by at most 4 B 2^-53 mean|x| <= 4 B 2^-53 max|x|, the larger of |minimum| and |maximum|
    u = 2.0 ** -53
    for grp in ("paths", "theta"):
        big = np.maximum(np.abs(full[f"{grp}/quantiles"][0]), np.abs(full[f"{grp}/quantiles"][-1]))
        assert np.all(np.abs(r0[f"{grp}/mean"] - full[f"{grp}/mean"]) <= 4.0 * P * u * big), grp
