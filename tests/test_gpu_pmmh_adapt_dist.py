"""theta_mcmc(adapt=True) and volatility_mcmc(adapt=True) over data-parallel ranks (on tests/test_gpu_pmmh_dist.py's
pattern): 2 ranks share cuda:0 over gloo, each rank a fresh child process.  The draw of q(theta) that sets the starting
factor and the chains' starts is rank 0's, broadcast; every rank then runs the identical deterministic launches, chained
through chol_end with the freeze inside the second, so both hold the same adaptive result, bit for bit."""
import numpy as np
import pytest

from tests import test_gpu_pmmh_dist as AD
from tests import test_gpu_svpmmh_dist as SD
from tests.dist_util import attach, run_ranks
from tests.parity_util import build_model

pytestmark = pytest.mark.gpu

MC, MN, MITER, MBURN = 6, 64, 12, 7         # five iterations per launch: the adaptation ends inside the second
KEYS = AD.KEYS + ("mcmc/prop_chol_end", "mcmc/accept_rate_adapt")


def _ar_worker(rank, world):
    from viforssms_amd import diagnostics
    diagnostics.MCMC_LAUNCH_STEPS = 5 * AD.T
    model = attach(AD._model(), rank, world, AD.P)
    res = model.theta_mcmc(MC, MN, MITER, MBURN, adapt=True)
    return {k: res[k] for k in KEYS}


def _sv_worker(rank, world):
    from viforssms_amd import diagnostics
    diagnostics.MCMC_LAUNCH_STEPS = 5 * SD.T
    model = attach(build_model("sv", *SD.SHAPE, "cuda:0", T=SD.T, precision=0, seed=3), rank, world, SD.P)
    res = model.volatility_mcmc(MC, MN, MITER, MBURN, adapt=True)
    return {k: res[k] for k in KEYS}


@pytest.mark.parametrize("worker,P", [(_ar_worker, 3), (_sv_worker, 4)])
def test_two_ranks_hold_identical_adaptive_chains(worker, P):
    res = run_ranks(worker)      # both children have exited (exit codes checked) before this process touches the GPU
    assert res[0]["mcmc/theta"].shape == (MC, MITER - MBURN, P) and res[0]["mcmc/prop_chol_end"].shape == (MC, P, P)
    assert np.all(np.diagonal(res[0]["mcmc/prop_chol_end"], axis1=1, axis2=2) > 0)
    assert not np.array_equal(res[0]["mcmc/prop_chol_end"][0], res[0]["mcmc/prop_chol"].astype(np.float32))
    for k in KEYS:
        assert np.array_equal(res[0][k], res[1][k], equal_nan=True), k
