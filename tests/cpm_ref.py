"""A numpy reference for the correlated pseudo-marginal chain of the stochastic-volatility model (include/vissm.h
vissm_sv_filter_sorted, vissm_sv_cpmmh; csrc/cpm_math.hpp), built on tests/svf_ref.py (the model), tests/pf_ref.py (the
integer resampling) and tests/pmmh_ref.py (the prior, the bars) by import.

* cn(), sigma_of(), sort_key(), key_value(), resample_u(): the contract's arithmetic, bit for bit (numpy float32,
  math.erfc).
* sort_states(): the sorted array of one step, fp32 bits: ascending, -0 before +0, everything not finite the quiet NaN
  and last.
* run_sorted_filter(): K filters in float64 on given move normals un [K, T, N] and resampling normals ur [K, T].
* cpm_chain(): C free-running correlated chains on that filter and a numpy Generator.
* ratio_noise(): the sd of D = ll(aux') - ll(aux) over K filters at one theta: what the sort and the correlation buy."""
import functools
import math

import numpy as np

from tests import pf_ref as PR
from tests import pmmh_ref as MR
from tests import svf_ref as SR

DEAD_KEY = np.uint32(0xFFFFFFFF)
_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def sigma_of(rho):
    """float32(sqrt(1 - rho^2)) with rho the fp32 value, the root in float64."""
    r = float(np.float32(rho))
    return np.float32(math.sqrt(1.0 - r * r))


def cn(u, eps, rho):
    """fl32(fl32(rho u) + fl32(sigma eps)) in numpy float32: every operation rounds on its own."""
    u, eps = np.asarray(u, np.float32), np.asarray(eps, np.float32)
    a = np.float32(rho) * u
    b = sigma_of(rho) * eps
    return (a + b).astype(np.float32)


def sort_key(h):
    b = np.ascontiguousarray(h, np.float32).view(np.uint32)
    k = np.where(b & np.uint32(0x80000000), ~b, b ^ np.uint32(0x80000000))
    return np.where((b & np.uint32(0x7F800000)) == np.uint32(0x7F800000), DEAD_KEY, k).astype(np.uint32)


def key_value(k):
    k = np.ascontiguousarray(k, np.uint32)
    b = np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32)
    return np.where(k == DEAD_KEY, np.float32(np.nan), b.view(np.float32)).astype(np.float32)


def sort_states(h):
    """The step's sorted array [..., N] fp32 (sorted along the last axis)."""
    return key_value(np.sort(sort_key(h), axis=-1))


def resample_u(ur):
    """min(2^24 - 1, floor(Phi(ur) 2^24)), Phi(x) = erfc(-x / sqrt 2) / 2 in float64 (math.erfc)."""
    x = np.asarray(ur, np.float32).astype(np.float64)
    s = np.floor(0.5 * _erfc(-x * 0.70710678118654752440) * 16777216.0)
    return np.minimum(s, 16777215.0).astype(np.int64)


def run_sorted_filter(theta, h0, y, dt, N, un, ur, sort=True, exp_dtype=np.float32):
    """K filters in float64: theta [K, 4], h0 a scalar or [K, N], y [T + 1], un [K, T, N], ur [K, T].  Each step sorts the
    states (sort=False: vissm_sv_filter's order, for the comparison), weighs, resamples with resample_u(ur) in integers
    and moves position j's ancestor with un[:, t, j].  Returns loglik [K] (-inf: dead)."""
    theta = np.asarray(theta, np.float64)
    K, T = theta.shape[0], len(y) - 1
    h = np.broadcast_to(np.asarray(h0, np.float64), (K, N)).copy()
    th = theta[:, None, :]
    ll, dead = np.zeros(K), np.zeros(K, bool)
    U = resample_u(ur).astype(np.uint64)
    for t in range(T):
        if sort:
            h = np.sort(h, axis=1)                     # NaN last
        alive = np.isfinite(h)
        m, q = PR.quantise(SR.state_logw(h, y[t], y[t + 1], th, dt), alive, exp_dtype)
        anc, W = PR.systematic_u64(q, U[:, t])
        dead |= W == 0
        with np.errstate(divide="ignore", invalid="ignore"):
            inc = m + np.log(W.astype(np.float64)) - PR.SCALE_BITS * math.log(2.0) - math.log(N)
        h = SR.h_step(np.take_along_axis(h, anc, axis=1), th, dt, un[:, t, :])
        h[dead] = np.nan
        ll = np.where(dead, -np.inf, ll + np.where(dead, 0.0, inc))
    return ll


def cpm_chain(theta0, L, prior, h0, y, dt, N, n_iter, rho, rng, sort=True):
    """C free-running correlated pseudo-marginal chains in float64: the state is (theta, un [C, T, N], ur [C, T]); a
    proposal moves theta by the random walk and the normals by rho u + sqrt(1 - rho^2) eps, and all are taken or left
    together.  Returns dict(theta [C, n, P], loglik [C, n], accept [C, n])."""
    theta = np.asarray(theta0, np.float64).copy()
    L, prior = np.asarray(L, np.float64), np.asarray(prior, np.float64)
    C, P = theta.shape
    T = len(y) - 1
    s = math.sqrt(1.0 - rho * rho)
    un, ur = rng.standard_normal((C, T, N)), rng.standard_normal((C, T))
    ll, lp = run_sorted_filter(theta, h0, y, dt, N, un, ur, sort), MR._log_prior_batch(theta, prior)
    out, lls, accs = np.empty((C, n_iter, P)), np.empty((C, n_iter)), np.zeros((C, n_iter), np.int32)
    for i in range(n_iter):
        prop = theta + rng.standard_normal((C, P)) @ L.T
        unp = rho * un + s * rng.standard_normal((C, T, N))
        urp = rho * ur + s * rng.standard_normal((C, T))
        llp, lpp = run_sorted_filter(prop, h0, y, dt, N, unp, urp, sort), MR._log_prior_batch(prop, prior)
        with np.errstate(invalid="ignore"):
            a = np.log(rng.uniform(size=C)) < (llp - ll) + (lpp - lp)
        theta[a], ll[a], lp[a], un[a], ur[a] = prop[a], llp[a], lpp[a], unp[a], urp[a]
        out[:, i], lls[:, i], accs[:, i] = theta, ll, a
    return {"theta": out, "loglik": lls, "accept": accs}


# ----------------------------------------------------------------------------------------------------------------
# the noise of the ratio: the first 257 values of dat/SV.dat at PARAM_INIT, h_0 = -8.5, dt = 1
# ----------------------------------------------------------------------------------------------------------------
NOISE_T, NOISE_N, NOISE_K, NOISE_H0, NOISE_DT = 256, 64, 256, -8.5, 1.0


def noise_series(root):
    """The first 257 values of the series the model fits: dat/SV.dat from entry 300 on (viforssms_amd.data.load_sv)."""
    import os
    y = np.loadtxt(os.path.join(root, "dat", "SV.dat"), dtype=np.float64).reshape(-1)[300:]
    return y[:NOISE_T + 1].astype(np.float32)


def ratio_noise(loglik, rho, seed, K=NOISE_K, T=NOISE_T, N=NOISE_N):
    """sd over K filters of D = ll(aux') - ll(aux), aux fresh N(0, 1) and aux' = cn(aux, fresh normals, rho) in fp32;
    loglik(un [K, T, N] fp32, ur [K, T] fp32) -> [K] is the filter under test (the reference's, or the GPU's)."""
    rng = np.random.default_rng(seed)
    un, ur = rng.standard_normal((K, T, N)).astype(np.float32), rng.standard_normal((K, T)).astype(np.float32)
    unp = cn(un, rng.standard_normal((K, T, N)).astype(np.float32), rho)
    urp = cn(ur, rng.standard_normal((K, T)).astype(np.float32), rho)
    d = np.asarray(loglik(unp, urp), np.float64) - np.asarray(loglik(un, ur), np.float64)
    assert np.isfinite(d).all()
    return float(d.std(ddof=1))


@functools.lru_cache(maxsize=8)
def reference_ratio_noise(root, rho, seed):
    """ratio_noise of the numpy reference filter (computed once per session)."""
    y = noise_series(root).astype(np.float64)
    th = np.tile(np.asarray(SR.PARAM_INIT), (NOISE_K, 1))
    return ratio_noise(lambda un, ur: run_sorted_filter(th, NOISE_H0, y, NOISE_DT, NOISE_N, un.astype(np.float64),
                                                        ur.astype(np.float64)), rho, seed)
