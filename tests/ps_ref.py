"""References for the particle smoother (include/vissm.h vissm_particle_smooth; csrc/ps_math.hpp):

* the transition log-densities of AR, LV and FHN in float64 from their formulas (trans_logp: what em::*_trans return
  as .lp), and the selection of one backward draw in Python ints (select_ints) and vectorised in uint64 (select_u64);
* a numpy float64 forward-filtering backward-simulation smoother on top of pf_ref.run_filter(cloud=True) (ffbsi),
  free-running on its own numpy Generator;
* the exact Kalman filter and Rauch-Tung-Striebel smoother of an AR(1) chain with Gaussian, partially observed data
  from a known x0 (rts_ar); observation t sees the state after transition t, as in pf_ref.kalman_ar_loglik.

The integer contract: m = max over live particles of logw, q_i = trunc(exp(logw_i - m) 2^40) with the exp in fp32
(pf_ref.quantise), W = sum q_i, and with a 32-bit word U tau = (U W) >> 32, idx = #{i : C_i <= tau} for the inclusive
cumulative sum C in particle order; W = 0 gives no draw (idx -1, a NaN state)."""
import bisect
import functools
import math

import numpy as np

from tests import pf_ref as PR
from tests import sim_util as SU

LOG_2PI = math.log(2.0 * math.pi)


def trans_logp(model, x, xt, th, dt, dtype=np.float64):
    """log p(xt | x, theta) from the densities' formulas, in `dtype` arithmetic (float64: the reference; float32: the
    yardstick of what fp32 costs): x, xt [..., S] (broadcast against each other), th [..., P] raw."""
    ty = np.dtype(dtype).type
    x, xt, th = np.asarray(x, ty), np.asarray(xt, ty), np.asarray(th, ty)
    dt, half, log2pi = ty(dt), ty(0.5), ty(LOG_2PI)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if model == SU.AR:
            z = (xt[..., 0] - th[..., 1] * x[..., 0] - th[..., 0]) / np.exp(th[..., 2])
            return -half * z * z - th[..., 2] - half * log2pi
        x1, x2 = x[..., 0], x[..., 1]
        if model == SU.LV:
            e0, e1, e2 = np.exp(th[..., 0]), np.exp(th[..., 1]), np.exp(th[..., 2])
            Bv = e1 * x1 * x2
            A, Cc = e0 * x1 + Bv, Bv + e2 * x2
            q1 = xt[..., 0] - x1 - dt * (e0 * x1 - Bv)
            q2 = xt[..., 1] - x2 - dt * (Bv - e2 * x2)
            Dl = A * Cc - Bv * Bv
            quad = (Cc * q1 * q1 + ty(2.0) * Bv * q1 * q2 + A * q2 * q2) / (dt * Dl)
            return -half * np.log(dt * dt * Dl) - half * quad - log2pi
        assert model == SU.FHN
        m1 = x1 + dt * np.exp(th[..., 0]) * (x1 - x1 * x1 * x1 - x2 + th[..., 1])
        m2 = x2 + dt * (th[..., 2] * x1 - x2 + ty(1.4))
        s1, s2 = np.sqrt(dt * np.exp(th[..., 3])), np.sqrt(dt * np.exp(th[..., 4]))
        z1, z2 = (xt[..., 0] - m1) / s1, (xt[..., 1] - m2) / s2
        return -half * (z1 * z1 + z2 * z2) - np.log(s1) - np.log(s2) - log2pi


def select_ints(q, U):
    """One backward draw in Python ints: q a sequence of non-negative ints, U < 2^32 -> (idx, W, tau); W = 0:
    (-1, 0, 0)."""
    q = [int(v) for v in q]
    assert 0 <= int(U) < 1 << 32
    C, W = [], 0
    for v in q:
        W += v
        C.append(W)
    if W == 0:
        return -1, 0, 0
    tau = (int(U) * W) >> 32
    return bisect.bisect_right(C, tau), W, tau


def select_u64(q, U):
    """The same for q [..., N] uint64 (q <= 2^40, W < 2^51) and U [...] < 2^32, vectorised: with W's low 25 bits w0
    and the rest w1, (U W) >> 32 = (U w1 + ((U w0) >> 25)) >> 7 exactly (nested floors; both products below 2^58).
    Returns (idx [...] int64, -1 where W = 0, and W)."""
    q = np.asarray(q, np.uint64)
    C = np.cumsum(q, axis=-1, dtype=np.uint64)
    W = C[..., -1]
    U = np.asarray(U, np.uint64)
    w0, w1 = W & np.uint64((1 << 25) - 1), W >> np.uint64(25)
    tau = (U * w1 + ((U * w0) >> np.uint64(25))) >> np.uint64(7)
    idx = (C <= tau[..., None]).sum(-1).astype(np.int64)
    return np.where(W > 0, idx, -1), W


def backward_draw(model, x, xt, th, dt, U, terminal=False):
    """One teacher-forced step for one filter: particles x [N, S] (float64), targets xt [M, S], th [P], U [M] ->
    (alive [N], logw [M, N] float64 (the full density; 0 at the terminal step), m [M], q [M, N] uint64, idx [M])."""
    alive = SU.alive(model, x)
    M = len(U)
    if terminal:
        lw = np.zeros((M, x.shape[0]))
    else:
        lw = trans_logp(model, x[None, :, :], np.asarray(xt, np.float64)[:, None, :], th, dt)
    ok = np.broadcast_to(alive[None, :], lw.shape) & ~np.isnan(lw)
    m, q = PR.quantise(np.where(ok, lw, -np.inf), ok)
    idx, _ = select_u64(q, U)
    return alive, lw, m, q, idx


def ffbsi(model, theta, cloud, dt, M, rng):
    """Backward simulation over cloud [K, N, S, T] (float64, the equally weighted post-resampling particles of
    pf_ref.run_filter): M trajectories per filter, [K, M, S, T]; NaN where no particle could be drawn."""
    theta = np.asarray(theta, np.float64)
    K, N, S, T = cloud.shape
    out = np.full((K, M, S, T), np.nan)
    xt = None
    for t in range(T - 1, -1, -1):
        U = rng.integers(0, 1 << 32, (K, M), dtype=np.uint64)
        nxt = np.empty((K, M, S))
        for k0 in range(0, K, 16):                                # (blocks of filters: the [k, M, N] temporaries fit a cache)
            sl = slice(k0, min(k0 + 16, K))
            x = cloud[sl, :, :, t]                                # k N S
            alive = SU.alive(model, x)
            if xt is None:
                lw = np.zeros((x.shape[0], M, N))
            else:
                lw = trans_logp(model, x[:, None, :, :], xt[sl, :, None, :], theta[sl, None, None, :], dt)
            ok = np.broadcast_to(alive[:, None, :], lw.shape) & ~np.isnan(lw)
            _, q = PR.quantise(np.where(ok, lw, -np.inf), ok)
            idx, _ = select_u64(q, U[sl])
            got = np.take_along_axis(x, np.maximum(idx, 0)[:, :, None], axis=1)
            nxt[sl] = np.where((idx >= 0)[:, :, None], got, np.nan)
        xt = nxt
        out[:, :, :, t] = xt
    return out


def rts_ar(theta, x0, obs, obs_bin, obs_std):
    """Exact Kalman filter and RTS smoother of x_{t+1} = th1 x_t + th0 + e^th2 n_t from a known x0, y_t = x_t +
    obs_std noise where obs_bin[t] != 0.  obs, obs_bin [T] -> dict(mf, vf: filtering mean and variance; ms, vs:
    smoothing)."""
    c, phi, s2 = float(theta[0]), float(theta[1]), math.exp(2.0 * float(theta[2]))
    r = float(obs_std) ** 2
    T = len(obs)
    mp, vp, mf, vf = np.zeros(T), np.zeros(T), np.zeros(T), np.zeros(T)
    m, v = float(x0), 0.0
    for t in range(T):
        m, v = phi * m + c, phi * phi * v + s2
        mp[t], vp[t] = m, v
        if obs_bin[t] != 0:
            g = v / (v + r)
            m, v = m + g * (float(obs[t]) - m), (1.0 - g) * v
        mf[t], vf[t] = m, v
    ms, vs = mf.copy(), vf.copy()
    for t in range(T - 2, -1, -1):
        J = vf[t] * phi / vp[t + 1]
        ms[t] = mf[t] + J * (ms[t + 1] - mp[t + 1])
        vs[t] = vf[t] + J * J * (vs[t + 1] - vp[t + 1])
    return {"mf": mf, "vf": vf, "ms": ms, "vs": vs}


# ----------------------------------------------------------------------------------------------------------------
# the statistical case: pf_ref's AR fixture (T = 64, obs_std = 1), theta = TRUE_THETA[AR], K = 256 filters of N = 256
# particles, M = 64 trajectories each
# ----------------------------------------------------------------------------------------------------------------
STAT_K, STAT_N, STAT_M = 256, 256, 64
MEAN_BAR = 0.2              # (b) |mean - RTS mean| in smoothing sds, at every step
SD_BAR = (0.85, 1.15)       # (c) pooled sd / RTS sd, at every step


def stat_rts():
    obs, obs_bin = PR.stat_case()
    return rts_ar(SU.TRUE_THETA[SU.AR], SU.TRUE_X[SU.AR][0], obs[0], obs_bin[0], 1.0)


def stat_moments(paths):
    """paths [K, M, T] -> (mean [T] over filters of the per-filter means, se [T] = across-filter sd / sqrt(K),
    pooled sd [T] of all K M trajectories).  NaN trajectories are not expected here."""
    K = paths.shape[0]
    pk = paths.mean(1)
    return pk.mean(0), pk.std(0, ddof=1) / math.sqrt(K), paths.reshape(-1, paths.shape[2]).std(0)


def stat_bars(mean, se, sd, mean_r, se_r, rts):
    """Conditions (a)-(c) as a dict of (passed, worst figure)."""
    s = np.sqrt(rts["vs"])
    a = np.abs(mean - mean_r) / (4.0 * np.sqrt(se * se + se_r * se_r))
    b = np.abs(mean - rts["ms"]) / s
    c = sd / s
    return {"a": (bool(np.all(a <= 1.0)), float(a.max())), "b": (bool(np.all(b <= MEAN_BAR)), float(b.max())),
            "c": (bool(np.all((c >= SD_BAR[0]) & (c <= SD_BAR[1]))), (float(c.min()), float(c.max())))}


@functools.lru_cache(maxsize=4)
def reference_paths(seed, K=STAT_K, N=STAT_N, M=STAT_M):
    """[K, M, T] trajectories of the reference smoother on the statistical case (computed once per session)."""
    obs, obs_bin = PR.stat_case()
    th = np.tile(np.asarray(SU.TRUE_THETA[SU.AR]), (K, 1))
    rng = np.random.default_rng(seed)
    r = PR.run_filter(SU.AR, th, SU.TRUE_X[SU.AR], obs, obs_bin, SU.DT[SU.AR], 1.0, N, rng, cloud=True)
    out = ffbsi(SU.AR, th, r["cloud"], SU.DT[SU.AR], M, rng)[:, :, 0, :]
    out.setflags(write=False)
    return out
