"""volatility_filter and volatility_smoother over data-parallel ranks: 2 ranks share cuda:0 over gloo (spawned as in
tests/test_gpu_particle_dist.py; each rank a fresh child process).  theta is rank 0's first rows of the first window's
draw, broadcast; every rank then runs the identical deterministic launches, so both hold, bit for bit, the result of
one process holding the full batch."""
import numpy as np
import pytest

from tests.dist_util import attach, run_ranks
from tests.parity_util import build_model

pytestmark = pytest.mark.gpu

P = 14
SHAPE, T = (P, 40, 8, 2, 16, 5, 3), 80      # SV: (B, M, k, n_flows, H, n_layers, fw), two windows
KF, NF, MF, CHUNK = 6, 128, 64, 30          # K <= p_local = 7; three launches per rank


def _model():
    return build_model("sv", *SHAPE, "cuda:0", T=T, precision=0, seed=3)


def _worker(rank, world):
    model = attach(_model(), rank, world, P)
    return model.volatility_smoother(KF, NF, MF, chunk=CHUNK)


def test_two_rank_volatility_smoother_equals_single_process():
    res = run_ranks(_worker)      # both children have exited (exit codes checked) before this process touches the GPU
    full = _model().volatility_smoother(KF, NF, MF)
    eq = lambda a, b: np.array_equal(a, b, equal_nan=np.asarray(a).dtype.kind == "f")
    assert str(full["filter/proposal"]) == "adapted" and np.isfinite(full["filter/loglik"]).any()
    assert full["filter/ll_inc"].shape == (KF, T) and full["smooth/quantiles"].shape == (5, 1, T)
    flt = _model().volatility_filter(KF, NF)
    for k in full:
        assert eq(res[0][k], res[1][k]), k
        assert eq(res[0][k], full[k]), k
        if k in flt:
            assert eq(flt[k], full[k]), k
