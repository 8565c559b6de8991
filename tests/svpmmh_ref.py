"""A numpy reference for particle marginal Metropolis-Hastings on the stochastic-volatility model (include/vissm.h
vissm_sv_pmmh), built on tests/pmmh_ref.py (the contract's integers and double arithmetic, the chain, the bars),
tests/svf_ref.py (the model, its numpy filter and its grid pass) and tests/pf_ref.py by import.

* iteration(): what one iteration of one chain must propose and draw -- theta', lp', log u -- from its Philox row.
* pmmh_chain(): C free-running chains on svf_ref.run_filter and a numpy Generator.
* grid_loglik_batch(): svf_ref.grid_pass's forward half for theta [C, 4] at once.  The transition matrix on the grid
  does not depend on t, so one [C, G, G] matrix per call and T - 1 mat-vecs suffice.
* exact_chain(): the same chain on that log-likelihood: the truth tests/golden/svpmmh_truth.npz records.

The statistical case is svf_ref's series (T = 64, dt = 1, h_0 = -8.5) under the prior N(PARAM_INIT, PRIOR_SD^2).  Flat
N(0, 10^2) priors let the chains wander to where the stationary level of h leaves any fixed grid; under this one a
uniform grid of 313 points on [-24, 2] agrees with 625 points and with 865 points on [-32, 4] to 1e-6 (the fixture keeps
the three values on 256 of its own draws; svf_ref.grid_pass's own range [-16, 1] is off by up to 4e-5 there)."""
import math
import os

import numpy as np

from tests import pmmh_ref as MR
from tests import svf_ref as SR

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svpmmh_truth.npz")
P = 4
PRIOR_SD = (0.05, 0.2, 0.3, 0.3)
GRID = (313, -24.0, 2.0)                             # the truth's grid
GRID_CHECKS = ((313, -24.0, 2.0), (625, -24.0, 2.0), (865, -32.0, 4.0))


def stat_prior():
    """[4, 2] fp32 (mean, sd): what the kernel takes."""
    return np.stack([np.asarray(SR.PARAM_INIT), np.asarray(PRIOR_SD)], 1).astype(np.float32)


def stat_series():
    return SR.fixture()["y"].astype(np.float64)


# ----------------------------------------------------------------------------------------------------------------
# the contract: one iteration
# ----------------------------------------------------------------------------------------------------------------
def iteration(seed, row0, i, C, c, N, theta, L, prior):
    """Iteration i of chain c from the state theta [4] fp32: (r, theta' fp32 [4], lp', log u).  The proposal takes the
    first four of the row's eight normals (Box-Muller in float64 here; the kernel's hardware transcendentals differ in
    the last bits, which is why the GPU test replays with a factor of small rows)."""
    r = MR.row_of(row0, i, C, c, N)
    thp = MR.propose(theta, L, MR.xi(seed, r)[:P])
    return r, thp, MR.log_prior(thp, prior), MR.log_u(seed, r)


# ----------------------------------------------------------------------------------------------------------------
# free-running chains
# ----------------------------------------------------------------------------------------------------------------
def pmmh_chain(theta0, L, prior, h0, y, dt, N, n_iter, rng):
    """C free-running PMMH chains on the numpy SV filter (svf_ref.run_filter) and the Generator rng."""
    def loglik(th):
        return SR.run_filter(th, h0, y, dt, N, rng)["loglik"]
    return MR._chain(loglik, theta0, L, prior, n_iter, rng)


def grid_loglik_batch(theta, h0, y, dt, n_grid=GRID[0], lo=GRID[1], hi=GRID[2]):
    """log p(y_1:T | y_0, h_0, theta) for theta [C, 4] on a uniform grid of h: svf_ref.grid_pass's forward recursion
    (rectangle rule), batched.  NaN where theta takes the arithmetic out of range (a chain rejects it)."""
    th = np.asarray(theta, np.float64)
    y = np.asarray(y, np.float64)
    T = len(y) - 1
    g = np.linspace(lo, hi, n_grid)
    dg = g[1] - g[0]
    with np.errstate(all="ignore"):
        # F[c, i, j] = f(g_j | g_i; theta_c) dg
        F = np.exp(SR.trans_logp(g[None, :, None], g[None, None, :], th[:, None, None, :], dt)) * dg
        ll = SR.state_logw(np.float64(h0), y[0], y[1], th, dt).astype(np.float64)
        alpha = np.exp(SR.trans_logp(np.float64(h0), g[None, :], th[:, None, :], dt)) * dg
        alpha = alpha / alpha.sum(1, keepdims=True)
        for t in range(1, T):
            a = alpha * np.exp(SR.state_logw(g[None, :], y[t], y[t + 1], th[:, None, :], dt))
            c = a.sum(1, keepdims=True)
            ll = ll + np.log(c[:, 0])
            nxt = np.matmul((a / c)[:, None, :], F)[:, 0, :]
            alpha = nxt / nxt.sum(1, keepdims=True)
    return ll


def exact_chain(theta0, L, prior, h0, y, dt, n_iter, rng, grid=GRID):
    """The chain on the grid log-likelihood: the truth."""
    def loglik(th):
        ll = grid_loglik_batch(th, h0, y, dt, *grid)
        return np.where(np.isnan(ll), -np.inf, ll)
    return MR._chain(loglik, theta0, L, prior, n_iter, rng)


# ----------------------------------------------------------------------------------------------------------------
# the fixture
# ----------------------------------------------------------------------------------------------------------------
def stat_start(t, C, seed):
    """C starting states spread as the posterior: start + chol(Sigma) z with chol(Sigma) = L / (2.38 / sqrt(4)), fp32."""
    z = np.random.default_rng(seed).standard_normal((C, P))
    return (t["start"].astype(np.float64) + z @ (t["L"].astype(np.float64) / (2.38 / math.sqrt(P))).T
            ).astype(np.float32)


def truth(acc="exact"):
    """The fixture's entries: L, prior [4, 2], start [4], mean, sd, se of the exact chain, and the acceptance `acc`
    asks for: "exact" the exact chain's, "ref64" the numpy PMMH reference's at N = 64 (the estimate's noise lowers the
    acceptance itself, so a PMMH run is compared with the reference at its own N, never with the exact chain)."""
    with np.load(FIXTURE) as z:
        t = {k: z[k] for k in ("L", "prior", "start", "mean", "sd", "se")}
        t["acc"] = z["acc"] if acc == "exact" else z[f"{acc}_acc"]
    return t
