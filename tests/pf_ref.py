"""Two references for the bootstrap particle filter (include/vissm.h vissm_particle_filter; csrc/pf_math.hpp):

* a numpy float64 restatement of the filter -- the Euler-Maruyama step of tests/sim_util.py, the observation density
  from its formula, the weights quantised to integers and systematic resampling in Python ints -- usable free-running
  on its own numpy Generator (run_filter) and teacher-forced on given states (weigh, systematic_ints);
* the exact Kalman log-likelihood of an AR(1) chain with Gaussian, partially observed data (kalman_ar_loglik).

The integer contract: m = max over live particles of logw, q_i = trunc(exp(logw_i - m) 2^40) with the exp in fp32,
W = sum q_i, ll_inc = m + log W - 40 ln 2 - ln N, ess = W^2 / sum q_i^2, and with a 24-bit integer U
tau_j = ((j 2^24 + U) W) >> (24 + log2 N), anc[j] = #{i : C_i <= tau_j} for the inclusive cumulative sum C."""
import bisect
import functools
import math
import os

import numpy as np

from tests import sim_util as SU

SCALE_BITS = 40
U_BITS = 24
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pf_ar_series.npz")


def obs_logw(x, y, b, sd):
    """sum_d b_d log N(y_d; x_d, sd) over the coordinates with b_d != 0, in float64.  x [..., S]; y, b [S]."""
    x = np.asarray(x, np.float64)
    lw = np.zeros(x.shape[:-1])
    for d in range(x.shape[-1]):
        if b[d] != 0:
            z = (x[..., d] - float(y[d])) / float(sd)
            lw = lw + float(b[d]) * (-0.5 * z * z - math.log(float(sd)) - HALF_LOG_2PI)
    return lw


def quantise(logw, alive, exp_dtype=np.float32):
    """(m, q) for logw [..., N] float64 and alive [..., N]: m = the maximum over the live particles (-inf if none),
    q = trunc(exp(logw - m) 2^40) as uint64, 0 for a dead particle and where no live particle has a finite weight.
    The difference is rounded to exp_dtype and exponentiated there (float32: the contract; float64: what an exact exp
    would give)."""
    lw = np.where(alive, logw, -np.inf)
    m = lw.max(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp((lw - m[..., None]).astype(exp_dtype)).astype(exp_dtype)
        v = (e * exp_dtype(2.0 ** SCALE_BITS)).astype(np.float64)
    v = np.where(np.isfinite(v) & alive, v, 0.0)
    return m, np.floor(v).astype(np.uint64)


def systematic_ints(q, U):
    """Systematic resampling in Python ints: q a sequence of N non-negative ints (N a power of two), U < 2^24 ->
    (anc list, W).  W = 0: (None, 0)."""
    q = [int(v) for v in q]
    N = len(q)
    log2n = N.bit_length() - 1
    assert 1 << log2n == N and 0 <= int(U) < 1 << U_BITS
    C, W = [], 0
    for v in q:
        W += v
        C.append(W)
    if W == 0:
        return None, 0
    anc = [bisect.bisect_right(C, (((j << U_BITS) + int(U)) * W) >> (U_BITS + log2n)) for j in range(N)]
    return anc, W


def systematic_u64(q, U):
    """The same for q [K, N] uint64 (q < 2^41, so W < 2^51) and U [K], vectorised: the 84-bit product is formed from
    W's 25-bit halves, (a W) >> s = (a w1 + ((a w0) >> 25)) >> (s - 25) exactly (nested floors; a < 2^34, so both
    partial products stay below 2^59).  Returns (anc [K, N] int64, W [K] uint64); rows with W = 0 get the identity."""
    q = np.asarray(q, np.uint64)
    K, N = q.shape
    log2n = N.bit_length() - 1
    assert 1 << log2n == N
    C = np.cumsum(q, axis=1, dtype=np.uint64)
    W = C[:, -1]
    a = (np.arange(N, dtype=np.uint64)[None, :] << np.uint64(U_BITS)) + np.asarray(U, np.uint64)[:, None]
    w0, w1 = W & np.uint64((1 << 25) - 1), W >> np.uint64(25)
    tau = (a * w1[:, None] + ((a * w0[:, None]) >> np.uint64(25))) >> np.uint64(U_BITS + log2n - 25)
    anc = np.empty((K, N), np.int64)
    for k in range(K):
        anc[k] = np.searchsorted(C[k], tau[k], side="right") if W[k] > 0 else np.arange(N)
    return anc, W


def ll_increment(m, W, N):
    return float(m) + math.log(int(W)) - SCALE_BITS * math.log(2.0) - math.log(N)


def ess(q):
    """W^2 / sum q^2 from exact integer sums."""
    q = [int(v) for v in q]
    W, s2 = sum(q), sum(v * v for v in q)
    return (W * W) / s2 if s2 else float("nan")


def weigh(model, x, y, b, obs_std, exp_dtype=np.float32):
    """Teacher-forced weighting of given states x [N, S] (float64): (alive, logw, m, q uint64 [N])."""
    alive = SU.alive(model, x)
    lw = obs_logw(x, y, b, obs_std)
    m, q = quantise(lw, alive, exp_dtype)
    return alive, lw, float(m), q


def run_filter(model, theta, x0, obs, obs_bin, dt, obs_std, N, rng, exp_dtype=np.float32, cloud=False):
    """K free-running filters in float64 on the Generator rng: theta [K, P], x0 [S], obs / obs_bin [S, T].
    Returns dict(loglik [K], ll_inc [K, T], ess [K, T], cloud [K, N, S, T] if asked)."""
    theta = np.asarray(theta, np.float64)
    K, S, T = theta.shape[0], SU.S_OF[model], obs.shape[1]
    x = np.broadcast_to(np.asarray(x0, np.float64), (K, N, S)).copy()
    x[~SU.alive(model, x)] = np.nan
    th = theta[:, None, :]
    ll, dead = np.zeros(K), np.zeros(K, bool)
    incs, esss = np.zeros((K, T)), np.full((K, T), float(N))
    out = np.full((K, N, S, T), np.nan) if cloud else None
    for t in range(T):
        x = SU.step(model, x, th, dt, rng.standard_normal((K, N, S)))
        x[~SU.alive(model, x)] = np.nan
        if np.any(obs_bin[:, t] != 0):
            alive = SU.alive(model, x)
            m, q = quantise(obs_logw(x, obs[:, t], obs_bin[:, t], obs_std), alive, exp_dtype)
            U = rng.integers(0, 1 << U_BITS, K, dtype=np.uint64)
            anc, W = systematic_u64(q, U)
            ok = W > 0
            dead |= ~ok
            qf = q.astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                inc = m + np.log(W.astype(np.float64)) - SCALE_BITS * math.log(2.0) - math.log(N)
                es = W.astype(np.float64) ** 2 / (qf * qf).sum(1)
            x = np.take_along_axis(x, anc[:, :, None], axis=1)
            x[dead] = np.nan
            ll = np.where(dead, -np.inf, ll + np.where(ok, inc, 0.0))
            incs[:, t], esss[:, t] = inc, es
        incs[dead, t] = np.nan
        esss[dead, t] = np.nan
        if cloud:
            out[:, :, :, t] = x
    return {"loglik": ll, "ll_inc": incs, "ess": esss, "cloud": out}


def kalman_ar_loglik(theta, x0, obs, obs_bin, obs_std):
    """Exact log p(y) of x_{t+1} = th1 x_t + th0 + e^th2 n_t from a known x0, y_t = x_t + obs_std noise observed
    where obs_bin[t] != 0 (observation t sees the state after transition t).  obs, obs_bin [T]."""
    c, phi, s2 = float(theta[0]), float(theta[1]), math.exp(2.0 * float(theta[2]))
    r = float(obs_std) ** 2
    mean, var, ll = float(x0), 0.0, 0.0
    for t in range(len(obs)):
        mean, var = phi * mean + c, phi * phi * var + s2
        if obs_bin[t] != 0:
            f = var + r
            e = float(obs[t]) - mean
            ll += -0.5 * (math.log(2.0 * math.pi * f) + e * e / f)
            g = var / f
            mean, var = mean + g * e, (1.0 - g) * var
    return ll


def ar_dataset(T=64, frac=0.7, obs_std=1.0, seed=0):
    """An AR(1) series at sim_util.TRUE_THETA[AR] from x0 = TRUE_X[AR], observed with N(x, obs_std) noise at about
    `frac` of the steps: (obs [1, T], obs_bin [1, T]) float32, unobserved entries 0."""
    rng = np.random.default_rng(seed)
    th = SU.TRUE_THETA[SU.AR]
    x, xs = float(SU.TRUE_X[SU.AR][0]), np.zeros(T)
    for t in range(T):
        x = th[1] * x + th[0] + math.exp(th[2]) * rng.standard_normal()
        xs[t] = x
    b = (rng.uniform(size=T) < frac).astype(np.float32)
    y = np.where(b > 0, xs + obs_std * rng.standard_normal(T), 0.0).astype(np.float32)
    return y[None, :], b[None, :]


# ----------------------------------------------------------------------------------------------------------------
# the statistical case: AR, T = 64, N = 256, theta = TRUE_THETA[AR], obs_std = 1, about 70 % of the steps observed
# (tests/golden/pf_ar_series.npz = ar_dataset(seed = its "seed" entry))
# ----------------------------------------------------------------------------------------------------------------
def stat_case():
    z = np.load(FIXTURE)
    return z["obs"], z["obs_bin"]


def stat_bars(mu, s, K, mu_r, s_r, K_r, L):
    """The three conditions on a sample of K log-likelihood estimates (mean mu, sd s) against the reference's K_r
    (mu_r, s_r) and the exact value L, as a dict of booleans: the means agree within four standard errors; the sd
    ratio lies in [0.8, 1.25] (four standard errors of an sd ratio at K = 256, K_r = 1024); L - mu lies between
    -4 se and s_r^2 + 4 se (Jensen puts the estimator's log below L by about s^2 / 2)."""
    se = math.sqrt(s * s / K + s_r * s_r / K_r)
    return {"mean": abs(mu - mu_r) <= 4.0 * se, "sd": 0.8 <= s / s_r <= 1.25,
            "kalman": -4.0 * se <= L - mu <= s_r * s_r + 4.0 * se}


@functools.lru_cache(maxsize=4)
def reference_logliks(seed, K=1024, N=256):
    """loglik [K] of K free-running reference filters on the statistical case (computed once per session)."""
    obs, obs_bin = stat_case()
    th = np.tile(np.asarray(SU.TRUE_THETA[SU.AR]), (K, 1))
    r = run_filter(SU.AR, th, SU.TRUE_X[SU.AR], obs, obs_bin, SU.DT[SU.AR], 1.0, N, np.random.default_rng(seed))
    r["loglik"].setflags(write=False)
    return r["loglik"]


def stat_kalman():
    obs, obs_bin = stat_case()
    return kalman_ar_loglik(SU.TRUE_THETA[SU.AR], SU.TRUE_X[SU.AR][0], obs[0], obs_bin[0], 1.0)
