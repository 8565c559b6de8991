"""References for the stochastic-volatility particle filter and smoother (include/vissm.h vissm_sv_filter,
vissm_sv_smooth; csrc/svf_math.hpp), numpy float64 unless a dtype is given:

* the weight log p(y_now | y_prev, h), the move of h and its transition density from their formulas;
* the filter -- weight the pre-step states, resample in integers (tests/pf_ref.py), move -- teacher-forced on given
  states (weigh) and free-running on its own numpy Generator (run_filter);
* forward filtering, backward simulation with the extra weight term (backward_draw, ffbsi; the integer selection of
  tests/ps_ref.py);
* a grid forward-backward pass over h (grid_pass): the near-exact log-evidence log p(y_1:T | y_0, h_0) and the means
  and sds of p(h_t | y_0:T).  It is truth only where two grid sizes agree (fixture_truth checks 1e-6).

The model, theta raw = (th0, th1, th2, th3):
  y_t | y_t-1, h_t-1 ~ N(y_t-1 (1 + dt th0), dt y_t-1^2 e^{h_t-1}),   h_t | h_t-1 ~ N(h_t-1 + dt (th1 - e^th2 h_t-1),
  dt e^{2 th3}).
Column t of a cloud, of the trajectories and of the grid moments holds h_t+1."""
import functools
import math
import os

import numpy as np

from tests import pf_ref as PR
from tests import ps_ref as PS

HALF_LOG_2PI = PR.HALF_LOG_2PI
PARAM_INIT = [0.001, -0.6, math.log(0.08), math.log(0.5)]      # viforssms_amd.sv.PARAM_INIT
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svf_series.npz")
FIX_T, FIX_DT, FIX_H0, FIX_Y0, FIX_N, FIX_K = 64, 1.0, -8.5, 1.0, 256, 1024


def state_logw(h, y_prev, y_now, th, dt, dtype=np.float64):
    """log N(y_now; y_prev (1 + dt th0), dt y_prev^2 e^h) in `dtype`; h [...], th [..., 4] broadcast; -inf where h is
    not finite."""
    ty = np.dtype(dtype).type
    h, th = np.asarray(h, ty), np.asarray(th, ty)
    y_prev, y_now, dt = ty(y_prev), ty(y_now), ty(dt)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        r = y_now - y_prev - dt * th[..., 0] * y_prev
        s = np.sqrt(dt) * np.abs(y_prev)
        z = r / s
        lw = -ty(HALF_LOG_2PI) - np.log(s) - ty(0.5) * h - ty(0.5) * z * z * np.exp(-h)
    return np.where(np.isfinite(h), lw, -np.inf)


def h_mean(h, th, dt):
    return h + dt * (th[..., 1] - np.exp(th[..., 2]) * h)


def h_step(h, th, dt, n, dtype=np.float64):
    """The next h from standard normals n, in `dtype`; NaN where the result is not finite."""
    ty = np.dtype(dtype).type
    h, th, n = np.asarray(h, ty), np.asarray(th, ty), np.asarray(n, ty)
    with np.errstate(invalid="ignore", over="ignore"):
        out = h + ty(dt) * (th[..., 1] - np.exp(th[..., 2]) * h) + np.sqrt(ty(dt)) * np.exp(th[..., 3]) * n
    return np.where(np.isfinite(out), out, np.nan)


def trans_logp(h, xt, th, dt, dtype=np.float64):
    """log f(xt | h) in `dtype`."""
    ty = np.dtype(dtype).type
    h, xt, th = np.asarray(h, ty), np.asarray(xt, ty), np.asarray(th, ty)
    with np.errstate(invalid="ignore", over="ignore"):
        sd = np.sqrt(ty(dt)) * np.exp(th[..., 3])
        z = (xt - h_mean(h, th, ty(dt))) / sd
        return -ty(0.5) * z * z - np.log(sd) - ty(HALF_LOG_2PI)


def weigh(h, y_prev, y_now, th, dt, exp_dtype=np.float32):
    """Teacher-forced weighting of the pre-step states h [N] of one filter: (alive, logw, m, q uint64 [N])."""
    h = np.asarray(h, np.float64)
    alive = np.isfinite(h)
    lw = state_logw(h, y_prev, y_now, np.asarray(th, np.float64), dt)
    m, q = PR.quantise(lw, alive, exp_dtype)
    return alive, lw, float(m), q


def run_filter(theta, h0, y, dt, N, rng, exp_dtype=np.float32, cloud=False):
    """K free-running filters on the Generator rng: theta [K, 4], h0 a scalar, y [T + 1].  Returns dict(loglik [K],
    ll_inc [K, T], ess [K, T], cloud [K, N, T] if asked)."""
    theta = np.asarray(theta, np.float64)
    K, T = theta.shape[0], len(y) - 1
    h = np.full((K, N), float(h0))
    th = theta[:, None, :]
    ll, dead = np.zeros(K), np.zeros(K, bool)
    incs, esss = np.zeros((K, T)), np.zeros((K, T))
    out = np.full((K, N, T), np.nan) if cloud else None
    for t in range(T):
        alive = np.isfinite(h)
        m, q = PR.quantise(state_logw(h, y[t], y[t + 1], th, dt), alive, exp_dtype)
        U = rng.integers(0, 1 << PR.U_BITS, K, dtype=np.uint64)
        anc, W = PR.systematic_u64(q, U)
        dead |= W == 0
        qf = q.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            inc = m + np.log(W.astype(np.float64)) - PR.SCALE_BITS * math.log(2.0) - math.log(N)
            es = W.astype(np.float64) ** 2 / (qf * qf).sum(1)
        h = h_step(np.take_along_axis(h, anc, axis=1), th, dt, rng.standard_normal((K, N)))
        h[dead] = np.nan
        ll = np.where(dead, -np.inf, ll + np.where(dead, 0.0, inc))
        incs[:, t], esss[:, t] = np.where(dead, np.nan, inc), np.where(dead, np.nan, es)
        if cloud:
            out[:, :, t] = h
    return {"loglik": ll, "ll_inc": incs, "ess": esss, "cloud": out}


def backward_logw(h, xt, th, dt, y_next, y_next2, dtype=np.float64):
    """The full backward weight log f(xt | h_i) + state_logw(h_i, y_next, y_next2): h [..., N], xt [..., 1]."""
    return trans_logp(h, xt, th, dt, dtype) + state_logw(h, y_next, y_next2, th, dt, dtype)


def backward_draw(h, xt, th, dt, y_next, y_next2, U, terminal=False):
    """One teacher-forced backward step for one filter: particles h [N], targets xt [M], th [4], U [M] -> (alive [N],
    logw [M, N] (0 at the terminal step), m [M], q [M, N] uint64, idx [M])."""
    h = np.asarray(h, np.float64)
    alive = np.isfinite(h)
    M = len(U)
    if terminal:
        lw = np.zeros((M, h.shape[0]))
    else:
        lw = backward_logw(h[None, :], np.asarray(xt, np.float64)[:, None], np.asarray(th, np.float64), dt, y_next,
                           y_next2)
    ok = np.broadcast_to(alive[None, :], lw.shape) & ~np.isnan(lw)
    m, q = PR.quantise(np.where(ok, lw, -np.inf), ok)
    idx, _ = PS.select_u64(q, U)
    return alive, lw, m, q, idx


def ffbsi(theta, cloud, y, dt, M, rng):
    """Backward simulation over cloud [K, N, T] of run_filter (column t = h_t+1): [K, M, T], NaN where no particle
    could be drawn."""
    theta = np.asarray(theta, np.float64)
    K, N, T = cloud.shape
    out = np.full((K, M, T), np.nan)
    xt = None
    for t in range(T - 1, -1, -1):
        U = rng.integers(0, 1 << 32, (K, M), dtype=np.uint64)
        nxt = np.empty((K, M))
        for k0 in range(0, K, 16):
            sl = slice(k0, min(k0 + 16, K))
            h = cloud[sl, :, t]
            alive = np.isfinite(h)
            if xt is None:
                lw = np.zeros((h.shape[0], M, N))
            else:
                lw = backward_logw(h[:, None, :], xt[sl, :, None], theta[sl, None, None, :], dt, y[t + 1], y[t + 2])
            ok = np.broadcast_to(alive[:, None, :], lw.shape) & ~np.isnan(lw)
            _, q = PR.quantise(np.where(ok, lw, -np.inf), ok)
            idx, _ = PS.select_u64(q, U[sl])
            got = np.take_along_axis(h, np.maximum(idx, 0), axis=1)
            nxt[sl] = np.where(idx >= 0, got, np.nan)
        xt = nxt
        out[:, :, t] = xt
    return out


def grid_pass(theta, h0, y, dt, n_grid, lo=-16.0, hi=1.0):
    """Forward-backward over a uniform grid of n_grid points of h on [lo, hi] (rectangle rule; the densities are
    smooth and vanish at both ends): dict(loglik = log p(y_1:T | y_0, h_0), ms, sds [T] = mean and sd of
    p(h_t+1 | y_0:T) at column t, mf, sdf [T] the same of the filtering law p(h_t+1 | y_0:t+1))."""
    th = np.asarray(theta, np.float64)
    T = len(y) - 1
    g = np.linspace(lo, hi, n_grid)
    dg = g[1] - g[0]
    # F[i, j] = f(g_j | g_i) dg
    F = np.exp(trans_logp(g[:, None], g[None, :], th, dt)) * dg
    # alpha_t(h_t) = p(h_t | y_0:t) on the grid (normalised); step t multiplies by w_t(h_t) = p(y_t+1 | y_t, h_t)
    ll = state_logw(np.float64(h0), y[0], y[1], th, dt).item()
    alpha = np.exp(trans_logp(np.float64(h0), g, th, dt)) * dg          # p(h_1 | h_0, y_0:1): the move is blind to y
    alphas = [alpha / alpha.sum()]
    for t in range(1, T):
        w = np.exp(state_logw(g, y[t], y[t + 1], th, dt))
        a = alphas[-1] * w
        c = a.sum()
        ll += math.log(c)
        nxt = (a / c) @ F
        alphas.append(nxt / nxt.sum())
    # alphas[t] = p(h_t+1 | y_0:t+1); beta_t(h_t+1) prop. to p(y_t+2:T | h_t+1, y)
    beta = np.ones(n_grid)
    ms, sds, mf, sdf = np.zeros(T), np.zeros(T), np.zeros(T), np.zeros(T)
    for t in range(T - 1, -1, -1):
        if t < T - 1:
            w = np.exp(state_logw(g, y[t + 1], y[t + 2], th, dt))       # of h_t+1 for y_t+2
            beta = w * (F @ beta)
            beta /= beta.max()
        for pm, ps_, dens in ((ms, sds, alphas[t] * beta), (mf, sdf, alphas[t])):
            dens = dens / dens.sum()
            pm[t] = (dens * g).sum()
            ps_[t] = math.sqrt(max((dens * (g - pm[t]) ** 2).sum(), 0.0))
    return {"loglik": ll, "ms": ms, "sds": sds, "mf": mf, "sdf": sdf}


def simulate_series(T, theta, dt, h0, y0, rng):
    """y [T + 1] float32 and h [T + 1] from the model itself."""
    th = np.asarray(theta, np.float64)
    y, h = np.zeros(T + 1), np.zeros(T + 1)
    y[0], h[0] = y0, h0
    for t in range(T):
        y[t + 1] = y[t] + dt * th[0] * y[t] + math.sqrt(dt) * y[t] * math.exp(0.5 * h[t]) * rng.standard_normal()
        h[t + 1] = h[t] + dt * (th[1] - math.exp(th[2]) * h[t]) + math.sqrt(dt) * math.exp(th[3]) * rng.standard_normal()
    return y.astype(np.float32), h


# ----------------------------------------------------------------------------------------------------------------
# the statistical case (tests/golden/svf_series.npz, written by tests/golden/make_svf_fixture.py): T = 64 at
# PARAM_INIT, dt = 1, h_0 = -8.5, y_0 = 1
# ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def fixture():
    with np.load(FIXTURE) as z:
        d = {k: z[k] for k in z.files}
    for v in d.values():
        v.setflags(write=False)
    return d


def fixture_truth():
    """(L, ms, sds) of the grid pass, after checking that the fixture's two grid sizes agree to 1e-6."""
    z = fixture()
    assert abs(float(z["grid_loglik"][0]) - float(z["grid_loglik"][1])) <= 1e-6
    assert np.max(np.abs(z["grid_ms"][0] - z["grid_ms"][1])) <= 1e-6
    assert np.max(np.abs(z["grid_sds"][0] - z["grid_sds"][1])) <= 1e-6
    return float(z["grid_loglik"][1]), z["grid_ms"][1], z["grid_sds"][1]


@functools.lru_cache(maxsize=4)
def reference_logliks(seed, K=FIX_K, N=FIX_N):
    """loglik [K] of K free-running reference filters on the statistical case (computed once per session)."""
    z = fixture()
    th = np.tile(np.asarray(PARAM_INIT), (K, 1))
    r = run_filter(th, FIX_H0, z["y"].astype(np.float64), FIX_DT, N, np.random.default_rng(seed))
    r["loglik"].setflags(write=False)
    return r["loglik"]


@functools.lru_cache(maxsize=2)
def reference_paths(seed, K=PS.STAT_K, N=PS.STAT_N, M=PS.STAT_M):
    """[K, M, T] trajectories of the reference smoother on the statistical case (computed once per session)."""
    z = fixture()
    y = z["y"].astype(np.float64)
    th = np.tile(np.asarray(PARAM_INIT), (K, 1))
    rng = np.random.default_rng(seed)
    r = run_filter(th, FIX_H0, y, FIX_DT, N, rng, cloud=True)
    out = ffbsi(th, r["cloud"], y, FIX_DT, M, rng)
    out.setflags(write=False)
    return out


def smooth_bars(mean, sd, ms, sds):
    """Bars (b) and (c) of tests/ps_ref.py against the grid smoother instead of RTS, as (passed, worst figure)."""
    b = np.abs(mean - ms) / sds
    c = sd / sds
    return {"b": (bool(np.all(b <= PS.MEAN_BAR)), float(b.max())),
            "c": (bool(np.all((c >= PS.SD_BAR[0]) & (c <= PS.SD_BAR[1]))), (float(c.min()), float(c.max())))}
