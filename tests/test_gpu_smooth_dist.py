"""particle_smoother over data-parallel ranks: 2 ranks share cuda:0 over gloo (spawned as in
tests/test_gpu_particle_dist.py; each rank a fresh child process).  theta is rank 0's first rows of the first window's
draw, broadcast; every rank then runs the identical deterministic launches -- the filter forward, the backward
simulation over its kept clouds -- so both hold, bit for bit, the result of one process holding the full batch."""
import numpy as np
import pytest

from tests.dist_util import attach, run_ranks
from tests.parity_util import FILTER_KEYS, SMOOTH_KEYS, build_model, pin_theta

pytestmark = pytest.mark.gpu

P = 16
SHAPE, T = (P, 30, 5, 2, 20, 3, 4), 60     # AR: (B, M, k, n_flows, H, n_layers, fw), two windows
KF, NF, MF, CHUNK = 6, 128, 64, 25          # K <= p_local = 8; three launches each way per rank
KEYS = FILTER_KEYS + SMOOTH_KEYS


def _model():
    from tests.sim_util import AR, TRUE_THETA
    return pin_theta(build_model("ar", *SHAPE, "cuda:0", T=T, precision=0, seed=3), TRUE_THETA[AR])


def _worker(rank, world):
    model = attach(_model(), rank, world, P)
    res = model.particle_smoother(KF, NF, MF, chunk=CHUNK)
    return {k: res[k] for k in KEYS}


def test_two_rank_smoother_equals_single_process():
    res = run_ranks(_worker)      # both children have exited (exit codes checked) before this process touches the GPU
    full = _model().particle_smoother(KF, NF, MF)
    assert sorted(full) == sorted(KEYS) and np.isfinite(full["filter/loglik"]).any()
    assert full["smooth/mean"].shape == (1, T) and full["smooth/quantiles"].shape == (5, 1, T)
    assert full["smooth/n_valid"].max() > 0
    for k in KEYS:
        assert np.array_equal(res[0][k], res[1][k], equal_nan=True), k
        assert np.array_equal(res[0][k], full[k], equal_nan=True), k
