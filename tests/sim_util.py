"""numpy restatements of the forecast's Euler-Maruyama steps (viforssms_amd/csrc/sim_math.hpp; include/vissm.h
vissm_sde_simulate), in the dtype they are given: float64 is the reference, float32 the yardstick of what fp32
arithmetic costs.  Shared by tests/test_sim_host.py and the GPU tests of the kernel."""
import numpy as np

AR, LV, SV, FHN = 0, 1, 2, 3
S_OF = {AR: 1, LV: 2, SV: 2, FHN: 2}
P_OF = {AR: 3, LV: 3, SV: 4, FHN: 5}
# the data generators' true parameters, raw (logs where the density exponentiates them): hyperparameters.txt,
# data.lv_data_gen, data.fhn_data_gen; SV: a stable volatility process
TRUE_THETA = {AR: [5.0, 0.5, np.log(3.0)], LV: np.log([0.5, 0.0025, 0.3]).tolist(),
              SV: [0.0, -0.5, np.log(0.5), np.log(0.2)], FHN: [np.log(2.0), 1.0, 1.5, np.log(0.5), np.log(0.3)]}
TRUE_X = {AR: [10.0], LV: [100.0, 100.0], SV: [1.0, -1.0], FHN: [2.0, 3.0]}
DT = {AR: 1.0, LV: 0.1, SV: 0.1, FHN: 0.1}


def step_terms(model, x, th, dt, n):
    """The next state's terms: a list over coordinates of lists of at most four arrays whose sum is x'.  x [.., S],
    th [.., P], n [.., >= S]; arithmetic in x's dtype."""
    ty = x.dtype.type
    dt = ty(dt)
    sq = np.sqrt(dt)
    if model == AR:
        return [[th[..., 1] * x[..., 0], th[..., 0], np.exp(th[..., 2]) * n[..., 0]]]
    x1, x2 = x[..., 0], x[..., 1]
    if model == LV:
        e0, e1, e2 = np.exp(th[..., 0]), np.exp(th[..., 1]), np.exp(th[..., 2])
        Bv = e1 * (x1 * x2)
        A = e0 * x1 + Bv
        Cc = Bv + e2 * x2
        with np.errstate(invalid="ignore", divide="ignore"):
            a = np.sqrt(A)
            b = -Bv / a
            c = np.sqrt(Cc - b * b)
        return [[x1, dt * (e0 * x1 - Bv), sq * a * n[..., 0]],
                [x2, dt * (Bv - e2 * x2), sq * (b * n[..., 0]), sq * (c * n[..., 1])]]
    if model == SV:
        return [[x1, dt * th[..., 0] * x1, sq * x1 * np.exp(ty(0.5) * x2) * n[..., 0]],
                [x2, dt * (th[..., 1] - np.exp(th[..., 2]) * x2), sq * np.exp(th[..., 3]) * n[..., 1]]]
    return [[x1, dt * np.exp(th[..., 0]) * (x1 - x1 * x1 * x1 - x2 + th[..., 1]),
             sq * np.sqrt(np.exp(th[..., 3])) * n[..., 0]],
            [x2, dt * (th[..., 2] * x1 - x2 + ty(1.4)), sq * np.sqrt(np.exp(th[..., 4])) * n[..., 1]]]


def step(model, x, th, dt, n):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([sum(t[1:], t[0]) for t in step_terms(model, x, th, dt, n)], -1)


def alive(model, x):
    ok = np.isfinite(x).all(-1)
    return ok & (x > 0).all(-1) if model == LV else ok


def replay(model, x_start, th, dt, normals, H, obs_std=None, dtype=np.float64):
    """The chain of H steps from normals [B, H * NS] (NS = S, or 2 S with observations) in `dtype`, with the death
    rule: (x [B, S, H], y or None, x_end [B, S], prev and raw [B, S, H] = the state each step was taken from and its
    result before the death rule (the boundary margin of a decision), exit [B] = the first dead step, H if none, -1
    for a dead start)."""
    S = S_OF[model]
    NS = 2 * S if obs_std is not None else S
    B = x_start.shape[0]
    x = x_start.astype(dtype)
    th = th.astype(dtype)
    nn = normals.astype(dtype).reshape(B, -1, NS)
    xs = np.full((B, S, H), np.nan, dtype)
    ys = np.full((B, S, H), np.nan, dtype) if obs_std is not None else None
    raw = np.full((B, S, H), np.nan, dtype)      # the step's result before the death rule
    prev = np.full((B, S, H), np.nan, dtype)     # the state it was taken from
    dead = ~alive(model, x)
    exit_step = np.where(dead, -1, H)
    x = np.where(dead[:, None], np.nan, x)
    for t in range(H):
        prev[:, :, t] = x
        nx = step(model, x, th, dt, nn[:, t])
        raw[:, :, t] = nx
        now_dead = ~alive(model, nx)
        exit_step = np.where(now_dead & ~dead, t, exit_step)
        dead |= now_dead
        x = np.where(dead[:, None], np.nan, nx)
        xs[:, :, t] = x
        if ys is not None:
            ys[:, :, t] = x + dtype(obs_std) * nn[:, t, S:]
    return xs, ys, x, prev, raw, exit_step


# ----------------------------------------------------------------------------------------------------------------
# inputs, bit comparisons and bars shared by the particle filter tests (tests/test_gpu_particle.py,
# tests/test_gpu_adapted.py)
# ----------------------------------------------------------------------------------------------------------------
PF_SEED = 0x9F17E2
PF_OBS_STD = {AR: 1.0, LV: 1.0, FHN: 0.1}
PF_ONE = 1 << 40


def filter_inputs(model, K, N, rng):
    """theta [K, P] within 10 % of the generators' true values (AR theta_1 in [0.5, 0.95]) and start states [K N, S]
    within 10 % of theirs: tests/test_gpu_simulate.py's stable range."""
    P, S = P_OF[model], S_OF[model]
    true = np.asarray(TRUE_THETA[model])
    if model == AR:
        th = true * rng.uniform(0.9, 1.1, (K, P))
        th[:, 1] = rng.uniform(0.5, 0.95, K)
    elif model == LV:
        th = true + np.log(rng.uniform(0.9, 1.1, (K, P)))
    else:
        th = true * rng.uniform(0.9, 1.1, (K, P))
    x0 = np.asarray(TRUE_X[model]) * rng.uniform(0.9, 1.1, (K * N, S))
    return th.astype(np.float32), x0.astype(np.float32)


def filter_series(model, T, pattern, rng):
    """One float64 path from the true start at the true theta, observed with N(x, obs_std) noise -- "all": every
    coordinate at every step; "tenth": every coordinate at steps 9, 19, ..; "coord": the first coordinate only, at
    steps 2, 5, ..; "none": nothing.  Unobserved entries hold -1, as the data files do."""
    S = S_OF[model]
    th = np.asarray(TRUE_THETA[model], np.float64)
    x = np.asarray(TRUE_X[model], np.float64)
    path = np.zeros((S, T))
    for t in range(T):
        x = step(model, x, th, DT[model], rng.standard_normal(S))
        path[:, t] = x
    assert alive(model, path.T).all()
    b = np.zeros((S, T), np.float32)
    if pattern == "all":
        b[:] = 1.0
    elif pattern == "tenth":
        b[:, 9::10] = 1.0
    elif pattern == "coord":
        b[0, 2::3] = 1.0
    y = np.where(b > 0, path + PF_OBS_STD[model] * rng.standard_normal((S, T)), -1.0).astype(np.float32)
    return y, b


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype.itemsize == 8 else np.int32)


def same_bits(a, b, keys=("loglik", "ll_inc", "ess", "state_end", "cloud", "q", "anc")):
    for k in keys:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert np.array_equal(bits(a[k]), bits(b[k])), k


def state_bar(ref64, ref32):
    """tests/test_gpu_simulate.py's bar: 8 * max(e32, 2^-20 * column mean |ref64|) per column [S, H], and e32."""
    both = np.isfinite(ref64) & np.isfinite(ref32)
    e32 = float(np.max(np.abs(ref32.astype(np.float64) - ref64)[both])) if both.any() else 0.0
    with np.errstate(invalid="ignore"):
        scale = np.nan_to_num(np.nanmean(np.abs(ref64), axis=0), nan=0.0)
    return 8.0 * np.maximum(e32, 2.0 ** -20 * scale), e32


def resample_u(seed, t, r):
    from tests import philox_ref
    w = philox_ref.philox4x32_10([t, 1, r & 0xFFFFFFFF, r >> 32], [seed & 0xFFFFFFFF, seed >> 32])
    return int(w[0]) >> 8
