"""A numpy reference for the fully adapted particle filter (include/vissm.h vissm_particle_filter_adapted;
csrc/gp_math.hpp), built on tests/sim_util.py and tests/pf_ref.py.

The Euler-Maruyama step is x' = mu(x) + L(x) n, so the transition moments are read off the step itself: mu is the
step at n = 0 and column d of L the step at the d-th unit normal less mu; Sigma = L L^T.  With O the observed
coordinates (obs_bin != 0) and R = obs_std^2, the predictive and the conditional follow from numpy.linalg on the
general formulas -- not the closed forms of the header:

    S_O = Sigma_OO + R I,   logw = log N(y_O; mu_O, S_O),
    K = Sigma_.O S_O^-1,    m = mu + K (y_O - mu_O),   P = Sigma - K Sigma_O.,   x' = m + chol(P) n.

Everything runs in the dtype of the state it is given: float64 is the reference, float32 the yardstick of what fp32
arithmetic costs these formulas.  Usable free-running on its own numpy Generator (run_filter) and teacher-forced on
given states (weigh, propagate).  The integer half (quantised weights, systematic resampling) is pf_ref's."""
import functools
import math

import numpy as np

from tests import pf_ref as PR
from tests import sim_util as SU


def moments(model, x, th, dt):
    """(mu [..., S], Sigma [..., S, S]) of the transition from x [..., S] at th [..., P], in x's dtype."""
    S = SU.S_OF[model]
    th = np.asarray(th, x.dtype)
    zero = np.zeros(x.shape[:-1] + (2,), x.dtype)
    mu = SU.step(model, x, th, dt, zero)
    cols = []
    for d in range(S):
        e = zero.copy()
        e[..., d] = 1
        cols.append(SU.step(model, x, th, dt, e) - mu)
    L = np.stack(cols, -1)                      # [..., S, S], column d = the response to normal d
    return mu, L @ np.swapaxes(L, -1, -2)


def observed(b):
    return [d for d in range(len(b)) if b[d] != 0]


def predictive_logw(mu, Sigma, y, b, obs_std):
    """log N(y_O; mu_O, Sigma_OO + R I) per particle, in mu's dtype."""
    ty = mu.dtype.type
    O = observed(b)
    R = ty(obs_std) * ty(obs_std)
    S_O = Sigma[..., O, :][..., :, O] + R * np.eye(len(O), dtype=mu.dtype)
    r = (np.asarray(y, mu.dtype)[O] - mu[..., O])[..., None]
    with np.errstate(invalid="ignore"):
        quad = (np.swapaxes(r, -1, -2) @ np.linalg.solve(S_O, r))[..., 0, 0]
        logdet = np.linalg.slogdet(S_O)[1].astype(mu.dtype)
    return ty(-0.5) * quad - ty(0.5) * logdet - ty(0.5 * len(O) * math.log(2.0 * math.pi))


def conditional(mu, Sigma, y, b, obs_std):
    """(m [..., S], L [..., S, S] lower, P [..., S, S]) of p(x' | x, y), in mu's dtype.  A particle whose moments are
    not finite (a dead one) gets NaN."""
    ty = mu.dtype.type
    O = observed(b)
    R = ty(obs_std) * ty(obs_std)
    ok = np.isfinite(mu).all(-1) & np.isfinite(Sigma).all((-1, -2))
    eye = np.eye(mu.shape[-1], dtype=mu.dtype)
    mu_s, Sg = np.where(ok[..., None], mu, ty(1)), np.where(ok[..., None, None], Sigma, eye)
    S_O = Sg[..., O, :][..., :, O] + R * np.eye(len(O), dtype=mu.dtype)
    Kt = np.linalg.solve(S_O, Sg[..., O, :])                # S_O^-1 Sigma_O. = K^T
    r = (np.asarray(y, mu.dtype)[O] - mu_s[..., O])[..., None]
    m = mu_s + (np.swapaxes(Kt, -1, -2) @ r)[..., 0]
    P = Sg - np.swapaxes(Kt, -1, -2) @ Sg[..., O, :]
    P = ty(0.5) * (P + np.swapaxes(P, -1, -2))
    L = np.linalg.cholesky(P)
    nan = ty(np.nan)
    return (np.where(ok[..., None], m, nan), np.where(ok[..., None, None], L, nan),
            np.where(ok[..., None, None], P, nan))


def propagate(model, x, th, dt, y, b, obs_std, n):
    """The conditional draw from the (ancestor's) state x [..., S] with normals n [..., >= S], without the death
    rule, in x's dtype."""
    S = SU.S_OF[model]
    mu, Sigma = moments(model, x, th, dt)
    m, L, _ = conditional(mu, Sigma, y, b, obs_std)
    return m + (L @ np.asarray(n, x.dtype)[..., :S, None])[..., 0]


def weigh(model, x, th, dt, y, b, obs_std, exp_dtype=np.float32):
    """Teacher-forced weighting of the pre-step states x [N, S] float64: (alive, logw, m, q uint64 [N])."""
    alive = SU.alive(model, x)
    mu, Sigma = moments(model, np.where(alive[..., None], x, 1.0), th, dt)
    lw = predictive_logw(mu, Sigma, y, b, obs_std)
    m, q = PR.quantise(lw, alive, exp_dtype)
    return alive, lw, float(m), q


def run_filter(model, theta, x0, obs, obs_bin, dt, obs_std, N, rng, exp_dtype=np.float32, cloud=False):
    """K free-running adapted filters in float64 on the Generator rng, with pf_ref.run_filter's arguments, result and
    order of draws (the step's normals, then the resampling integers)."""
    theta = np.asarray(theta, np.float64)
    K, S, T = theta.shape[0], SU.S_OF[model], obs.shape[1]
    x = np.broadcast_to(np.asarray(x0, np.float64), (K, N, S)).copy()
    x[~SU.alive(model, x)] = np.nan
    th = np.broadcast_to(theta[:, None, :], (K, N, theta.shape[1]))
    ll, dead = np.zeros(K), np.zeros(K, bool)
    incs, esss = np.zeros((K, T)), np.full((K, T), float(N))
    out = np.full((K, N, S, T), np.nan) if cloud else None
    for t in range(T):
        n = rng.standard_normal((K, N, S))
        if np.any(obs_bin[:, t] != 0):
            alive = SU.alive(model, x)
            mu, Sigma = moments(model, np.where(alive[..., None], x, 1.0), th, dt)
            m, q = PR.quantise(predictive_logw(mu, Sigma, obs[:, t], obs_bin[:, t], obs_std), alive, exp_dtype)
            U = rng.integers(0, 1 << PR.U_BITS, K, dtype=np.uint64)
            anc, W = PR.systematic_u64(q, U)
            ok = W > 0
            dead |= ~ok
            qf = q.astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                inc = m + np.log(W.astype(np.float64)) - PR.SCALE_BITS * math.log(2.0) - math.log(N)
                es = W.astype(np.float64) ** 2 / (qf * qf).sum(1)
            xa = np.take_along_axis(x, anc[:, :, None], axis=1)
            xa[dead] = np.nan
            live = SU.alive(model, xa)
            x = np.full_like(xa, np.nan)
            if live.any():
                x[live] = propagate(model, xa[live], th[live], dt, obs[:, t], obs_bin[:, t], obs_std, n[live])
            ll = np.where(dead, -np.inf, ll + np.where(ok, inc, 0.0))
            incs[:, t], esss[:, t] = inc, es
        else:
            x = SU.step(model, x, th, dt, n)
        x[~SU.alive(model, x)] = np.nan
        incs[dead, t] = np.nan
        esss[dead, t] = np.nan
        if cloud:
            out[:, :, :, t] = x
    return {"loglik": ll, "ll_inc": incs, "ess": esss, "cloud": out}


@functools.lru_cache(maxsize=4)
def reference_logliks(seed, K=1024, N=256):
    """loglik [K] of K free-running adapted reference filters on pf_ref's statistical case (once per session)."""
    obs, obs_bin = PR.stat_case()
    th = np.tile(np.asarray(SU.TRUE_THETA[SU.AR]), (K, 1))
    r = run_filter(SU.AR, th, SU.TRUE_X[SU.AR], obs, obs_bin, SU.DT[SU.AR], 1.0, N, np.random.default_rng(seed))
    r["loglik"].setflags(write=False)
    return r["loglik"]


# ----------------------------------------------------------------------------------------------------------------
# the small two-coordinate cases: LV and FHN at sim_util.TRUE_THETA from TRUE_X, T = 40, observed every fifth step
# (steps 4, 9, ..), the coordinates of `mask` with N(x, obs_std) noise; data seed 1000 * model + index of the case
# ----------------------------------------------------------------------------------------------------------------
SMALL_T, SMALL_EVERY = 40, 5
SMALL_OBS_STD = {SU.LV: (10.0, 2.0), SU.FHN: (0.2, 0.05)}
SMALL_MASKS = ((1, 1), (1, 0), (0, 1))
SMALL_CASES = [(model, sd, mask) for model in (SU.LV, SU.FHN) for sd in SMALL_OBS_STD[model] for mask in SMALL_MASKS]


def small_dataset(model, obs_std, mask):
    """(obs, obs_bin) [2, 40] float32 of one case; unobserved entries hold -1, as the data files do."""
    seed = 1000 * model + SMALL_CASES.index((model, obs_std, tuple(mask)))
    rng = np.random.default_rng(seed)
    th = np.asarray(SU.TRUE_THETA[model], np.float64)
    x = np.asarray(SU.TRUE_X[model], np.float64)
    path = np.zeros((2, SMALL_T))
    for t in range(SMALL_T):
        x = SU.step(model, x, th, SU.DT[model], rng.standard_normal(2))
        path[:, t] = x
    assert SU.alive(model, path.T).all()
    b = np.zeros((2, SMALL_T), np.float32)
    for d in range(2):
        if mask[d]:
            b[d, SMALL_EVERY - 1::SMALL_EVERY] = 1.0
    y = np.where(b > 0, path + obs_std * rng.standard_normal((2, SMALL_T)), -1.0).astype(np.float32)
    return y, b


@functools.lru_cache(maxsize=16)
def small_logliks(model, obs_std, mask, proposal, K=256, N=256, seed=7):
    """loglik [K] of K free-running reference filters (proposal "adapted" or "bootstrap") on one small case."""
    obs, obs_bin = small_dataset(model, obs_std, mask)
    th = np.tile(np.asarray(SU.TRUE_THETA[model]), (K, 1))
    run = run_filter if proposal == "adapted" else PR.run_filter
    r = run(model, th, SU.TRUE_X[model], obs, obs_bin, SU.DT[model], obs_std, N,
            np.random.default_rng(seed + (0 if proposal == "adapted" else 1)))
    r["loglik"].setflags(write=False)
    return r["loglik"]


def jensen_bars(ll_a, ll_b):
    """-4 se <= mu_adapted - mu_bootstrap <= s_b^2 + 4 se: both estimate the same evidence without bias, so the means
    of their logs differ by the difference of their Jensen gaps, about (s_b^2 - s_a^2) / 2 >= 0."""
    mu_a, mu_b, s_a, s_b = ll_a.mean(), ll_b.mean(), ll_a.std(ddof=1), ll_b.std(ddof=1)
    se = math.sqrt(s_a * s_a / ll_a.size + s_b * s_b / ll_b.size)
    return {"mu_a": mu_a, "mu_b": mu_b, "s_a": s_a, "s_b": s_b, "se": se,
            "ok": -4.0 * se <= mu_a - mu_b <= s_b * s_b + 4.0 * se}
