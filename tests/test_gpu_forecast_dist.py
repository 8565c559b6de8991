"""forecast over data-parallel ranks: 2 ranks share cuda:0 over gloo (spawned as in tests/test_gpu_summary_dist.py;
each rank a fresh child process).  The forecast's Philox rows are keyed by the global sample index, like the draw it
starts from, so the two ranks' halves are together the trajectories of one process holding the full batch: quantiles
and n_valid are exact over their union, the means' double sums are reduced in another order, within the moments'
bound."""
import numpy as np
import pytest

from tests.dist_util import attach, run_ranks

pytestmark = pytest.mark.gpu

P = 16
SHAPE, T = (P, 30, 5, 2, 20, 3, 4), 60     # AR: (B, M, k, n_flows, H, n_layers, fw), two windows
PROBS = (0.0, 0.025, 0.5, 0.975, 1.0)       # with the extremes: max|x| per column bounds the means' error
HORIZON = 70                                 # two launches per rank at chunk = 64
KEYS = ("forecast/mean", "forecast/sd", "forecast/quantiles", "forecast/n_valid", "forecast/obs/mean",
        "forecast/obs/sd", "forecast/obs/quantiles", "forecast/obs/n_valid", "forecast/start")


def _model():
    from tests.parity_util import build_model
    return build_model("ar", *SHAPE, "cuda:0", T=T, precision=0, seed=3)


def _worker(rank, world):
    model = attach(_model(), rank, world, P)
    res = model.forecast(HORIZON, PROBS, obs=True, chunk=64)
    return {k: res[k] for k in KEYS}


def test_two_rank_forecast_equals_full_batch():
    res = run_ranks(_worker)      # both children have exited (exit codes checked) before this process touches the GPU
    full = _model().forecast(HORIZON, PROBS, obs=True)
    r0, r1 = res[0], res[1]
    for k in KEYS:
        assert np.array_equal(r0[k], r1[k], equal_nan=True), k          # replicated result: bitwise on both ranks
    for grp in ("forecast", "forecast/obs"):
        for k in ("quantiles", "n_valid"):
            assert np.array_equal(r0[f"{grp}/{k}"], full[f"{grp}/{k}"]), (grp, k)   # exact over the ranks' union
    assert full["forecast/quantiles"].shape == (5, 1, HORIZON) and np.all(full["forecast/n_valid"] == P)
    assert int(r0["forecast/start"]) == T
    # means: the two halves' sums added vs one pass, each within 2 B 2^-53 sum|x| of the exact sum, so the means
    # differ by at most 4 B 2^-53 mean|x| <= 4 B 2^-53 max|x|, the larger of |minimum| and |maximum|; the variances
    # E x^2 - mean^2 carry that bound in both terms: 8 (B + 2) 2^-53 max|x|^2 on either side
    u = 2.0 ** -53
    for grp in ("forecast", "forecast/obs"):
        big = np.maximum(np.abs(full[f"{grp}/quantiles"][0]), np.abs(full[f"{grp}/quantiles"][-1]))
        assert np.all(np.abs(r0[f"{grp}/mean"] - full[f"{grp}/mean"]) <= 4.0 * P * u * big), grp
        assert np.all(np.abs(r0[f"{grp}/sd"] ** 2 - full[f"{grp}/sd"] ** 2) <= 16.0 * (P + 2) * u * big * big), grp
