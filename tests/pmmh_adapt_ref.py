"""A numpy reference for the adaptive chains (include/vissm.h vissm_pmmh_adaptive; csrc/mh_math.hpp), written from the
header's text on top of tests/pmmh_ref.py.

* alpha(), eta() and adapt(): the acceptance probability, the step size and the rank-one update of one chain's factor,
  in float64 scalars in the header's order, so adapt() reproduces mh::adapt bit for bit.
* adapt_batch(): the same update for C chains at once (float64 throughout, the factor not rounded to fp32): the free
  running reference chains use it.
* adaptive_chain(): C free-running adaptive chains on any loglik(theta [C, P]) -> [C]; exact_ar_loglik() the Kalman
  likelihood of the AR fixture plus N(-1/2, 1) noise, the stand-in for a particle estimate of unit variance.
* bad_factor(): chol(D Sigma D), the recorded failure shape the statistical tests start from.
* stat_conditions(): the conditions of the statistical tests."""
import math

import numpy as np

from tests import pmmh_ref as MR

TARGET, GAMMA = 0.234, 0.5
F32_MAX = float(np.finfo(np.float32).max)


def alpha(ll_prop, ll_cur, lp_prop, lp_cur):
    """0 if r is NaN, 1 if r >= 0, else exp(r); r = (ll' - ll) + (lp' - lp), accept()'s expression."""
    with np.errstate(invalid="ignore"):
        r = (np.float64(ll_prop) - np.float64(ll_cur)) + (np.float64(lp_prop) - np.float64(lp_cur))
    if np.isnan(r):
        return 0.0
    return 1.0 if r >= 0.0 else float(np.exp(r))


def eta(P, i, gamma):
    """min(1, P (i + 1)^-gamma) of the absolute iteration i."""
    return min(1.0, float(P * np.power(np.float64(i + 1), -np.float64(gamma))))


def adapt(L, xi, al, et, target):
    """L [P, P] fp32 (lower) -> (L' fp32 with the upper part 0, changed).  Every guard hands back the input's lower
    part."""
    L = np.asarray(L, np.float32)
    P = L.shape[0]
    keep = np.tril(L).astype(np.float32)
    f = np.float64
    x = [f(np.float32(v)) for v in xi[:P]]
    d = f(et) * (f(al) - f(target))
    n2 = f(0.0)
    for j in range(P):
        n2 = n2 + x[j] * x[j]
    if not (n2 > 0.0) or d == 0.0 or not np.isfinite(d):
        return keep, False
    s = np.sqrt(np.abs(d) / n2)
    sgn = f(1.0) if d > 0.0 else f(-1.0)
    A = [[f(L[p, j]) for j in range(P)] for p in range(P)]
    v = []
    for p in range(P):
        w = f(0.0)
        for j in range(p + 1):
            w = w + A[p][j] * x[j]
        v.append(w * s)
    with np.errstate(all="ignore"):
        for k in range(P):
            r2 = A[k][k] * A[k][k] + sgn * (v[k] * v[k])
            if not (A[k][k] > 0.0) or not (r2 > 0.0):
                return keep, False
            rho = np.sqrt(r2)
            c, t = rho / A[k][k], v[k] / A[k][k]
            A[k][k] = rho
            for i in range(k + 1, P):
                A[i][k] = (A[i][k] + sgn * (t * v[i])) / c
                v[i] = c * v[i] - t * A[i][k]
        out = np.zeros((P, P), np.float32)
        for p in range(P):
            for j in range(p + 1):
                out[p, j] = np.float32(A[p][j])
    if not np.isfinite(out).all() or not (np.diag(out) > 0).all():
        return keep, False
    return out, True


def adapt_batch(L, xi, al, et, target):
    """The update of C chains at once in float64: L [C, P, P] (lower) -> L'.  A chain whose update is skipped or
    breaks down keeps its factor."""
    C, P, _ = L.shape
    d = et * (al - target)
    n2 = (xi * xi).sum(1)
    with np.errstate(all="ignore"):
        ok = (n2 > 0.0) & (d != 0.0) & np.isfinite(d)
        s = np.sqrt(np.abs(d) / np.where(ok, n2, 1.0))
        sgn = np.where(d > 0.0, 1.0, -1.0)
        A = L.copy()
        v = np.einsum("cpj,cj->cp", np.tril(L), xi) * s[:, None]
        for k in range(P):
            r2 = A[:, k, k] ** 2 + sgn * v[:, k] ** 2
            ok &= (A[:, k, k] > 0.0) & (r2 > 0.0)
            rho = np.sqrt(np.where(r2 > 0.0, r2, 1.0))
            c, t = rho / A[:, k, k], v[:, k] / A[:, k, k]
            A[:, k, k] = rho
            for i in range(k + 1, P):
                A[:, i, k] = (A[:, i, k] + sgn * t * v[:, i]) / c
                v[:, i] = c * v[:, i] - t * A[:, i, k]
        ok &= np.isfinite(A).all((1, 2)) & (np.diagonal(A, axis1=1, axis2=2) > 0.0).all(1)
    return np.where(ok[:, None, None], A, L)


def adaptive_chain(loglik, theta0, L0, prior, n_iter, adapt_end, rng, target=TARGET, gamma=GAMMA):
    """C adaptive random-walk chains in float64 on loglik(theta [C, P]) -> [C]: pmmh_ref._chain with a factor per
    chain that follows adapt_batch while i < adapt_end.  L0 [P, P] or [C, P, P]."""
    theta = np.asarray(theta0, np.float64).copy()
    C, P = theta.shape
    prior = np.asarray(prior, np.float64)
    L = np.broadcast_to(np.asarray(L0, np.float64), (C, P, P)).copy()
    ll, lp = loglik(theta), MR._log_prior_batch(theta, prior)
    out, accs = np.empty((C, n_iter, P)), np.zeros((C, n_iter), np.int32)
    for i in range(n_iter):
        xi = rng.standard_normal((C, P))
        prop = theta + np.einsum("cpj,cj->cp", L, xi)
        llp, lpp = loglik(prop), MR._log_prior_batch(prop, prior)
        with np.errstate(invalid="ignore", over="ignore"):
            r = (llp - ll) + (lpp - lp)
            a = np.log(rng.uniform(size=C)) < r
            al = np.where(np.isnan(r), 0.0, np.where(r >= 0.0, 1.0, np.exp(np.minimum(r, 0.0))))
        if i < adapt_end:
            L = adapt_batch(L, xi, al, eta(P, i, gamma), target)
        theta[a], ll[a], lp[a] = prop[a], llp[a], lpp[a]
        out[:, i], accs[:, i] = theta, a
    return {"theta": out, "accept": accs, "chol_end": L}


def exact_ar_loglik(x0, obs, obs_bin, obs_std, rng):
    """theta [C, 3] -> the exact Kalman log-likelihood of the AR model plus N(-1/2, 1) noise: an unbiased estimate of
    the likelihood with the variance of a particle estimate at a sensible N."""
    def loglik(th):
        return MR.kalman_ar_loglik_batch(th, x0, obs[0], obs_bin[0], obs_std) + rng.normal(-0.5, 1.0, th.shape[0])
    return loglik


def bad_factor(L, scale):
    """chol(D Sigma D) with Sigma = L L^T and D = diag(scale, 1, ..., 1): D L, which is lower with a positive
    diagonal already.  fp32."""
    D = np.ones(L.shape[0])
    D[0] = scale
    return (D[:, None] * np.asarray(L, np.float64)).astype(np.float32)


def stat_conditions(theta_kept, accept_kept, chol_end, truth, target=TARGET):
    """The conditions of the statistical tests on the kept draws [C, n, P]: pmmh_ref.stat_bars' mean and sd-ratio
    conditions against the truth (its acceptance condition does not apply: the adapted chain aims at `target`, not at
    the fixture's rate), pooled kept acceptance in [target / 2, 2 target], every chol_end finite with a positive
    diagonal."""
    s = MR.summarise(np.asarray(theta_kept, np.float64), accept_kept)
    bars = MR.stat_bars(s, truth)
    dm, ratio = bars["dmean_over_se"], bars["sd_ratio"]
    chol_ok = bool(np.isfinite(chol_end).all() and (np.diagonal(chol_end, axis1=1, axis2=2) > 0).all())
    acc_ok = bool(target / 2.0 <= s["acc"] <= 2.0 * target)
    ok = bool((dm <= 4.0).all() and (ratio >= 0.9).all() and (ratio <= 1.1).all() and acc_ok and chol_ok)
    return {"dmean_over_se": dm, "sd_ratio": ratio, "acc": s["acc"], "chol_ok": chol_ok, "ok": ok,
            "rhat": [MR.split_rhat(np.asarray(theta_kept, np.float64)[:, :, p]) for p in range(theta_kept.shape[2])]}
