"""A numpy reference for particle marginal Metropolis-Hastings (include/vissm.h vissm_pmmh; csrc/mh_math.hpp), built on
tests/philox_ref.py, tests/gpf_ref.py and tests/pf_ref.py.

* The contract's integers and its double arithmetic, restated from the header's text: the Philox words on counter
  (g, 2, lo32(r), hi32(r)), the uniform, Box-Muller in float64 rounded to fp32, the proposal summed in float64 in
  ascending order, the log-prior from subtract / divide / multiply / add, and the acceptance rule.
* replay(): the chain that follows from recorded proposals, their estimates and log u.
* pmmh_chain(): C free-running chains on gpf_ref.run_filter (the numpy adapted filter) and a numpy Generator.
* exact_chain(): the same chain on the exact Kalman log-likelihood of the AR model (kalman_ar_loglik_batch, checked
  against pf_ref.kalman_ar_loglik): the truth tests/golden/pmmh_ar_truth.npz records.
* split_rhat(): the split-R-hat of Gelman et al. (BDA3, section 11.4), written from its definition.
* stat_bars(): the three conditions of the statistical tests."""
import math
import os

import numpy as np

from tests import gpf_ref as GR
from tests import philox_ref

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pmmh_ar_truth.npz")
M64 = (1 << 64) - 1
PRIOR_CASES = ("flat", "informative")
STAT_X0, STAT_OBS_STD = 10.0, 1.0


# ----------------------------------------------------------------------------------------------------------------
# the contract
# ----------------------------------------------------------------------------------------------------------------
def row_of(row0, i, C, c, N):
    return (int(row0) + (int(i) * int(C) + int(c)) * int(N)) & M64


def words(seed, r, g):
    """The Philox block of group g of row r: uint64 [4] holding 32-bit words."""
    seed, r = int(seed) & M64, int(r) & M64
    return philox_ref.philox4x32_10([g, 2, r & 0xFFFFFFFF, r >> 32], [seed & 0xFFFFFFFF, seed >> 32])


def xi(seed, r):
    """The eight normals of row r, fp32: Box-Muller in float64 on groups 0 and 1, rounded."""
    w = np.stack([words(seed, r, 0), words(seed, r, 1)])
    return philox_ref.box_muller(philox_ref.uniforms(w), np.float64).reshape(8).astype(np.float32)


def uniform(x):
    """u = ((x >> 8) + 1/2) 2^-24 of a 32-bit word, float64 (exact)."""
    return (float(int(x) >> 8) + 0.5) * 2.0 ** -24


def log_u(seed, r):
    return math.log(uniform(words(seed, r, 2)[0]))


def propose(theta, L, z):
    """float32(theta_p + sum_{j <= p} L_pj z_j), float64, ascending j."""
    theta, L, z = np.asarray(theta, np.float32), np.asarray(L, np.float32), np.asarray(z, np.float32)
    out = np.empty(theta.shape[0], np.float32)
    for p in range(theta.shape[0]):
        s = np.float64(theta[p])
        for j in range(p + 1):
            s = s + np.float64(L[p, j]) * np.float64(z[j])
        out[p] = np.float32(s)
    return out


def log_prior(theta, prior):
    """-1/2 sum_p ((theta_p - m_p) / s_p)^2 in float64, ascending p; theta [P] fp32, prior [P, 2] fp32."""
    theta, prior = np.asarray(theta, np.float32), np.asarray(prior, np.float32)
    acc = np.float64(0.0)
    for p in range(theta.shape[0]):
        z = (np.float64(theta[p]) - np.float64(prior[p, 0])) / np.float64(prior[p, 1])
        acc = acc + z * z
    return float(np.float64(-0.5) * acc)


def accept(logu, ll_prop, ll_cur, lp_prop, lp_cur):
    with np.errstate(invalid="ignore"):
        return bool(np.float64(logu) < (np.float64(ll_prop) - np.float64(ll_cur)) +
                    (np.float64(lp_prop) - np.float64(lp_cur)))


def replay(theta0, ll0, prior, theta_prop, ll_prop, logu):
    """The chains that follow from the recorded proposals [C, n, P], their estimates and log u [C, n]:
    (theta_chain [C, n, P] fp32, ll_chain [C, n], accept [C, n] int32, theta_cur [C, n, P]: the state each proposal
    was made from)."""
    C, n, P = theta_prop.shape
    th_chain, cur = np.empty((C, n, P), np.float32), np.empty((C, n, P), np.float32)
    ll_chain, acc = np.empty((C, n)), np.zeros((C, n), np.int32)
    for c in range(C):
        th, ll = np.asarray(theta0[c], np.float32).copy(), float(ll0[c])
        lp = log_prior(th, prior)
        for i in range(n):
            cur[c, i] = th
            lpp = log_prior(theta_prop[c, i], prior)
            if accept(logu[c, i], ll_prop[c, i], ll, lpp, lp):
                th, ll, lp = theta_prop[c, i].copy(), float(ll_prop[c, i]), lpp
                acc[c, i] = 1
            th_chain[c, i], ll_chain[c, i] = th, ll
    return th_chain, ll_chain, acc, cur


# ----------------------------------------------------------------------------------------------------------------
# free-running chains
# ----------------------------------------------------------------------------------------------------------------
def _log_prior_batch(theta, prior):
    z = (theta - prior[:, 0]) / prior[:, 1]
    return -0.5 * (z * z).sum(-1)


def _chain(loglik, theta0, L, prior, n_iter, rng):
    """C random-walk Metropolis chains in float64 on loglik(theta [C, P]) -> [C] (noisy or exact)."""
    theta = np.asarray(theta0, np.float64).copy()
    L, prior = np.asarray(L, np.float64), np.asarray(prior, np.float64)
    C, P = theta.shape
    ll, lp = loglik(theta), _log_prior_batch(theta, prior)
    out, lls, accs = np.empty((C, n_iter, P)), np.empty((C, n_iter)), np.zeros((C, n_iter), np.int32)
    for i in range(n_iter):
        prop = theta + rng.standard_normal((C, P)) @ L.T
        llp, lpp = loglik(prop), _log_prior_batch(prop, prior)
        with np.errstate(invalid="ignore"):
            a = np.log(rng.uniform(size=C)) < (llp - ll) + (lpp - lp)
        theta[a], ll[a], lp[a] = prop[a], llp[a], lpp[a]
        out[:, i], lls[:, i], accs[:, i] = theta, ll, a
    return {"theta": out, "loglik": lls, "accept": accs}


def pmmh_chain(model, theta0, L, prior, x0, obs, obs_bin, dt, obs_std, N, n_iter, rng):
    """C free-running PMMH chains on the numpy adapted filter (gpf_ref.run_filter) and the Generator rng."""
    def loglik(th):
        return GR.run_filter(model, th, x0, obs, obs_bin, dt, obs_std, N, rng)["loglik"]
    return _chain(loglik, theta0, L, prior, n_iter, rng)


def kalman_ar_loglik_batch(theta, x0, obs, obs_bin, obs_std):
    """pf_ref.kalman_ar_loglik for theta [C, 3] at once."""
    theta = np.asarray(theta, np.float64)
    c, phi, s2 = theta[:, 0], theta[:, 1], np.exp(2.0 * theta[:, 2])
    r = float(obs_std) ** 2
    mean, var, ll = np.full(theta.shape[0], float(x0)), np.zeros(theta.shape[0]), np.zeros(theta.shape[0])
    for t in range(len(obs)):
        mean, var = phi * mean + c, phi * phi * var + s2
        if obs_bin[t] != 0:
            f = var + r
            e = float(obs[t]) - mean
            ll = ll - 0.5 * (np.log(2.0 * np.pi * f) + e * e / f)
            g = var / f
            mean, var = mean + g * e, (1.0 - g) * var
    return ll


def exact_chain(theta0, L, prior, x0, obs, obs_bin, obs_std, n_iter, rng):
    """The chain on the exact AR log-likelihood: the truth."""
    def loglik(th):
        return kalman_ar_loglik_batch(th, x0, obs[0], obs_bin[0], obs_std)
    return _chain(loglik, theta0, L, prior, n_iter, rng)


# ----------------------------------------------------------------------------------------------------------------
# summaries and bars
# ----------------------------------------------------------------------------------------------------------------
def split_rhat(x):
    """x [C, n] -> split-R-hat: each chain cut into halves (the middle draw of an odd n dropped), B the between- and W
    the within-half variance, sqrt(((m - 1) / m W + B / m) / W) with m draws per half."""
    x = np.asarray(x, np.float64)
    m = x.shape[1] // 2
    h = np.concatenate([x[:, :m], x[:, x.shape[1] - m:]], 0)
    W = h.var(axis=1, ddof=1).mean()
    B = m * h.mean(axis=1).var(ddof=1)
    return math.sqrt(((m - 1) / m * W + B / m) / W)


def summarise(theta, accept):
    """theta [C, n, P] kept draws, accept [C, n] -> mean, pooled sd, between-chain se of the mean [P], acceptance and
    its between-chain se."""
    C = theta.shape[0]
    cm = theta.mean(1)
    ar = accept.mean(1)
    return {"mean": cm.mean(0), "sd": theta.reshape(-1, theta.shape[2]).std(0, ddof=1),
            "se": cm.std(0, ddof=1) / math.sqrt(C), "acc": float(ar.mean()),
            "acc_se": float(ar.std(ddof=1) / math.sqrt(C))}


def stat_bars(s, truth):
    """|mean - truth| <= 4 sqrt(se^2 + se_truth^2) per coordinate; pooled sd ratio in [0.9, 1.1]; |acceptance - the
    truth's| <= 4 se between the run's chains.  s: summarise() of the run; truth: the fixture's entries."""
    dm = np.abs(s["mean"] - truth["mean"]) / np.sqrt(s["se"] ** 2 + truth["se"] ** 2)
    ratio = s["sd"] / truth["sd"]
    da = abs(s["acc"] - float(truth["acc"])) / s["acc_se"]
    return {"dmean_over_se": dm, "sd_ratio": ratio, "dacc_over_se": da,
            "ok": bool((dm <= 4.0).all() and (ratio >= 0.9).all() and (ratio <= 1.1).all() and da <= 4.0)}


def stat_start(t, C, seed):
    """C starting states spread as the posterior: start + chol(Sigma) z with chol(Sigma) = L / (2.38 / sqrt(3)), fp32."""
    z = np.random.default_rng(seed).standard_normal((C, 3))
    return (t["start"].astype(np.float64) + z @ (t["L"].astype(np.float64) / (2.38 / math.sqrt(3.0))).T
            ).astype(np.float32)


def truth(case):
    """The fixture's entries of one prior case: L, prior [3, 2], start [3], mean, sd, se, acc."""
    z = np.load(FIXTURE)
    return {k: z[f"{case}_{k}"] for k in ("L", "prior", "start", "mean", "sd", "se", "acc")}
