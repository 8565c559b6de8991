"""volatility_mcmc(correlation=0.99) over data-parallel ranks (modelled on tests/test_gpu_svpmmh_dist.py): 2 ranks share
cuda:0 over gloo, each rank a fresh child process.  The draw of q(theta) is rank 0's, broadcast; the carried normals
come from the Philox stream, so every rank starts the same chains, runs the identical deterministic launches and holds
the same result, bit for bit."""
import numpy as np
import pytest

from tests.dist_util import attach, run_ranks
from tests.parity_util import build_model

pytestmark = pytest.mark.gpu

P = 14
SHAPE, T = (P, 40, 8, 2, 16, 5, 3), 80      # SV: (B, M, k, n_flows, H, n_layers, fw), two windows
MC, MN, MITER, MBURN = 6, 64, 12, 3         # C <= p_local = 7
KEYS = ("mcmc/theta", "mcmc/loglik", "mcmc/accept_rate", "mcmc/prop_chol", "mcmc/mean", "mcmc/sd", "mcmc/quantiles",
        "mcmc/rhat", "mcmc/correlation", "theta/mean", "theta/sd", "theta/quantiles")


def _worker(rank, world):
    from viforssms_amd import diagnostics
    diagnostics.MCMC_LAUNCH_STEPS = 5 * T       # five iterations per launch: three launches per rank
    model = attach(build_model("sv", *SHAPE, "cuda:0", T=T, precision=0, seed=3), rank, world, P)
    res = model.volatility_mcmc(MC, MN, MITER, MBURN, correlation=0.99)
    return {k: res[k] for k in KEYS}


def test_two_ranks_hold_identical_chains():
    res = run_ranks(_worker)      # both children have exited (exit codes checked) before this process touches the GPU
    assert res[0]["mcmc/theta"].shape == (MC, MITER - MBURN, 4) and res[0]["mcmc/loglik"].shape == (MC, MITER - MBURN)
    for k in KEYS:
        assert np.array_equal(res[0][k], res[1][k], equal_nan=True), k
