"""vissm_particle_smooth (ops.particle_smooth) on the GPU.

Every chosen state is bitwise the cloud's particle the index names, and never a dead one.  Teacher-forced, step by
step against tests/ps_ref.py on the kernel's own next state: the index is the integer selection of the traced weights
(vectorised uint64, and Python ints on three lanes per step; U from tests/philox_ref.py) exactly, the traced weights
lie within the q bar of tests/test_gpu_particle.py of the float64 ones.  Constructed clouds pin the edge cases: one live
particle per step, a dead step, dead particles, the uniform terminal draw.  Chained, sub-batched and repeated calls
are compared bitwise.  The per-step means of 256 x 64 trajectories agree with the numpy reference and with the exact
RTS smoother within the bars tests/test_ps_host.py confirms for the reference alone.  VISSMBase.particle_smoother
equals the by-hand chain of calls."""
import math
import os

import numpy as np
import pytest
import torch

from tests import pf_ref as PR
from tests import philox_ref
from tests import ps_ref as PS
from tests import sim_util as SU
from tests.parity_util import FILTER_CASES as CASES, FILTER_KEYS, SMOOTH_KEYS, filter_model as _model

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5F00B5
ONE = 1 << 40
SPREAD = {SU.AR: 2.0, SU.LV: 2.0, SU.FHN: 0.1}      # particle scatter about the path: of the transition's own sd


def _theta(model, K, rng):
    """theta [K, P] within 10 % of the generators' true values (AR theta_1 in [0.5, 0.95])."""
    P = SU.P_OF[model]
    true = np.asarray(SU.TRUE_THETA[model])
    if model == SU.LV:
        th = true + np.log(rng.uniform(0.9, 1.1, (K, P)))
    else:
        th = true * rng.uniform(0.9, 1.1, (K, P))
    if model == SU.AR:
        th[:, 1] = rng.uniform(0.5, 0.95, K)
    return th.astype(np.float32)


def _cloud(model, K, N, H, rng):
    """A synthetic cloud [K N, S, H]: one float64 path from the true start at the true theta, every particle the
    path's state plus normal scatter of about the transition's sd, so a backward draw has many candidates."""
    S = SU.S_OF[model]
    th = np.asarray(SU.TRUE_THETA[model], np.float64)
    x = np.asarray(SU.TRUE_X[model], np.float64)
    path = np.zeros((S, H))
    for t in range(H):
        x = SU.step(model, x, th, SU.DT[model], rng.standard_normal(S))
        path[:, t] = x
    assert SU.alive(model, path.T).all()
    c = path[None] + SPREAD[model] * rng.standard_normal((K * N, S, H))
    if model == SU.LV:
        c = np.abs(c) + 1e-3
    return c.astype(np.float32)


def _smooth(model, th, cloud, M, row0=0, t0=0, x_next=None, idx=True, trace=False, seed=SEED):
    from viforssms_amd import ops
    g = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    r = ops.particle_smooth(model, g(th), g(cloud), SU.DT[model], M, seed, row0, t0=t0, x_next=g(x_next), idx=idx,
                            trace=trace)
    torch.cuda.synchronize()
    c = lambda t: None if t is None else t.cpu().numpy()
    return {"paths": c(r.paths), "x_first": c(r.x_first), "idx": c(r.idx), "q": c(r.q_trace)}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype.itemsize == 8 else np.int32)


def _same(a, b, keys=("paths", "x_first", "idx", "q")):
    for k in keys:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def _select_u(seed, t_abs, rows):
    """The selection words of Philox rows `rows` [..] (Python ints or uint64) at absolute step t_abs."""
    rows = np.asarray(rows, np.uint64)
    ctr = np.zeros(rows.shape + (4,), np.uint64)
    ctr[..., 0], ctr[..., 1] = t_abs, 2
    ctr[..., 2], ctr[..., 3] = rows & philox_ref.M32, rows >> philox_ref.SH32
    return philox_ref.philox4x32_10(ctr, np.asarray([seed & 0xFFFFFFFF, seed >> 32], np.uint64))[..., 0]


def _check(model, th, cloud, r, K, N, M, row0=0, t0=0, x_next=None, seed=SEED, q_steps=()):
    """The gather identity everywhere; with a trace the exact selection everywhere and the q bar at q_steps."""
    S, H, dt = SU.S_OF[model], cloud.shape[2], SU.DT[model]
    cl, paths, idx = cloud.reshape(K, N, S, H), r["paths"].reshape(K, M, S, H), r["idx"].reshape(K, M, H)
    assert np.array_equal(_bits(r["x_first"]), _bits(r["paths"][:, :, 0]))
    share = 0.0
    for k in range(K):
        for t in range(H - 1, -1, -1):
            x, ix = cl[k, :, :, t], idx[k, :, t].astype(np.int64)
            alive = SU.alive(model, x)
            drawn = ix >= 0
            assert np.all(ix[drawn] < N) and alive[ix[drawn]].all(), (k, t)
            assert np.array_equal(_bits(paths[k, drawn, :, t]), _bits(x[ix[drawn]])), (k, t)
            assert np.isnan(paths[k, ~drawn, :, t]).all(), (k, t)
            if r["q"] is None:
                continue
            terminal = t == H - 1 and x_next is None
            target = None if terminal else (paths[k, :, :, t + 1] if t < H - 1 else x_next.reshape(K, M, S)[k])
            U = _select_u(seed, t0 + t, row0 + k * N + np.arange(M))
            qk = r["q"][k, t].astype(np.uint64)
            want, W = PS.select_u64(qk, U)
            assert np.array_equal(ix, want), (k, t)
            for j in (0, M // 2 + 1, M - 1):
                assert PS.select_ints(qk[j], int(U[j]))[0] == ix[j], (k, t, j)
            assert not qk[:, ~alive].any() and np.all(qk.max(1)[W > 0] == ONE), (k, t)
            if t not in q_steps:
                continue
            th64 = th[k].astype(np.float64)
            _, lw64, m64, qref, _ = PS.backward_draw(model, x.astype(np.float64), None if terminal else
                                                     target.astype(np.float64), th64, dt, U, terminal)
            if terminal:
                lw32 = np.zeros_like(lw64, dtype=np.float32)
            else:
                lw32 = PS.trans_logp(model, x[None, :, :], target[:, None, :], th[k], dt, np.float32)
            live = np.broadcast_to(alive[None, :], lw64.shape) & np.isfinite(lw64)
            assert live.any()
            d = 8.0 * max(float(np.max(np.abs(lw32.astype(np.float64) - lw64)[live])),
                          2.0 ** -20 * float(np.mean(np.abs(lw64[live]))))
            qr = qref.astype(np.float64)
            with np.errstate(invalid="ignore"):
                gap = np.where(live, np.abs(lw64 - m64[:, None]), 0.0)
            tol = qr * (math.expm1(2.0 * d) + (gap + 2.0) * 2.0 ** -23) + 1.0
            err = np.abs(qk.astype(np.float64) - qr)
            assert np.all(err <= tol), (k, t, float(np.max(err / tol)))
            share = max(share, float(np.max(err / tol)))
    return share


# ----------------------------------------------------------------------------------------------------------------
# 1. gather identity and teacher-forced exactness
# ----------------------------------------------------------------------------------------------------------------
# (N, M) in {(64, 64), (128, 64), (1024, 1024)} x H in {1, 63, 64, 65, 131} x K in {1, 3}, pruned so that each case
# stays at a few seconds: the full-size block walks 63 .. 65 steps with one filter (the trace alone is 8 MiB a step)
@pytest.mark.parametrize("model,N,M,H,K", [
    (SU.AR, 64, 64, 131, 3), (SU.AR, 128, 64, 64, 1), (SU.AR, 1024, 1024, 63, 1), (SU.AR, 64, 64, 1, 3),
    (SU.LV, 64, 64, 63, 1), (SU.LV, 128, 64, 131, 3), (SU.LV, 1024, 1024, 65, 1), (SU.LV, 128, 64, 1, 1),
    (SU.FHN, 64, 64, 65, 3), (SU.FHN, 128, 64, 63, 1), (SU.FHN, 1024, 1024, 1, 3), (SU.FHN, 1024, 1024, 64, 1)])
def test_teacher_forced_selection(model, N, M, H, K):
    """Step t is checked from the kernel's own state at t + 1, so a decision is never second-guessed: given its
    traced weights the index must be the integer selection exactly.  Weights: the kernel's logw_i and m each lie
    within d = 8 * max(e32, 2^-20 mean |logw|) of the float64 ones (e32: the density in numpy float32 against
    float64), so exp(logw_i - m) is off by a factor within e^(2 d); the fp32 rounding of the difference and of the
    exp add (|logw_i - m| + 2) 2^-23 relative, the truncation one unit (tests/test_gpu_particle.py's q bar)."""
    rng = np.random.default_rng(1000 * model + 10 * N + H + K)
    th, cloud = _theta(model, K, rng), _cloud(model, K, N, H, rng)
    if N == 128:      # some dead particles: NaN, and for LV outside the orthant
        cloud[5::16, 0, :] = np.nan
        if model == SU.LV:
            cloud[9::16, 1, H // 2:] = -1.0
    row0, t0 = 2 ** 32 - 2 * N + 7, 3
    r = _smooth(model, th, cloud, M, row0=row0, t0=t0, trace=True)
    assert r["paths"].shape == (K * M, SU.S_OF[model], H) and r["q"].shape == (K, H, M, N)
    assert np.isfinite(r["paths"]).all() and (r["idx"] >= 0).all()
    big = N == 1024
    q_steps = sorted({0, H - 1, H // 2, max(H - 2, 0)}) if big else range(H)
    share = _check(model, th, cloud, r, K, N, M, row0=row0, t0=t0, q_steps=q_steps)
    print(f"model {model} N {N} M {M} H {H} K {K}: largest share of the q bar {share:.3f}")
    if H > 1:         # the draws differ between trajectories and use many particles
        assert len(np.unique(r["idx"][:, H // 2])) > min(N, K * M) // 8


# ----------------------------------------------------------------------------------------------------------------
# 2. constructed clouds
# ----------------------------------------------------------------------------------------------------------------
def test_one_live_particle_per_step_is_followed():
    model, K, N, M, H = SU.AR, 2, 128, 64, 37
    rng = np.random.default_rng(2)
    th, full = _theta(model, K, rng), _cloud(model, K, N, H, rng)
    live = rng.integers(0, N, (K, H))
    cloud = np.full_like(full, np.nan)
    for k in range(K):
        for t in range(H):
            cloud[k * N + live[k, t], :, t] = full[k * N + live[k, t], :, t]
    r = _smooth(model, th, cloud, M, trace=True)
    assert np.array_equal(r["idx"].reshape(K, M, H), np.broadcast_to(live[:, None, :], (K, M, H)))
    _check(model, th, cloud, r, K, N, M)
    assert np.all(r["q"].sum(3) == ONE)


def test_dead_step_kills_the_steps_before_it():
    """Filter 1 of 3 as a dead filter leaves its cloud -- NaN from step 20 on: all of its trajectories are NaN with
    idx -1, and its neighbours are the filters they are without it.  A single dead step in an otherwise live cloud
    gives NaN at that step and every earlier one (a NaN target has W = 0); the later steps were drawn before it."""
    model, K, N, M, H = SU.LV, 3, 64, 64, 45
    rng = np.random.default_rng(3)
    th, good = _theta(model, K, rng), _cloud(model, K, N, H, rng)
    ok = _smooth(model, th, good, M)
    cloud = good.copy()
    cloud[N:2 * N, :, 20:] = np.nan
    r = _smooth(model, th, cloud, M)
    assert np.isnan(r["paths"][M:2 * M]).all() and (r["idx"][M:2 * M] == -1).all()
    assert np.isnan(r["x_first"][M:2 * M]).all()
    for k in (0, 2):
        sl = slice(k * M, (k + 1) * M)
        for key in ("paths", "x_first", "idx"):
            assert np.array_equal(_bits(r[key][sl]), _bits(ok[key][sl])), (k, key)
    cloud = good.copy()
    cloud[N:2 * N, 0, 20] = -3.0                          # outside the orthant: dead for LV
    r = _smooth(model, th, cloud, M)
    assert np.isnan(r["paths"][M:2 * M, :, :21]).all() and (r["idx"][M:2 * M, :21] == -1).all()
    assert np.array_equal(_bits(r["paths"][M:2 * M, :, 21:]), _bits(ok["paths"][M:2 * M, :, 21:]))
    _check(model, th, cloud, r, K, N, M)
    # a NaN x_next does the same from the last step
    xn = ok["paths"][:, :, -1].copy()
    xn[5, 1] = np.nan
    r = _smooth(model, th, good, M, x_next=xn)
    assert np.isnan(r["paths"][5]).all() and (r["idx"][5] == -1).all() and np.isfinite(np.delete(r["paths"], 5, 0)).all()


def test_dead_particles_are_never_chosen():
    model, K, N, M, H = SU.LV, 2, 256, 128, 33
    rng = np.random.default_rng(4)
    th, cloud = _theta(model, K, rng), _cloud(model, K, N, H, rng)
    dead = rng.uniform(size=(K * N, H)) < 0.4
    cloud[:, 0, :] = np.where(dead & (rng.uniform(size=dead.shape) < 0.5), np.nan, cloud[:, 0, :])
    cloud[:, 1, :] = np.where(dead & np.isfinite(cloud[:, 0, :]), -cloud[:, 1, :], cloud[:, 1, :])
    assert 0.3 < (~SU.alive(model, cloud.transpose(0, 2, 1))).mean() < 0.5
    r = _smooth(model, th, cloud, M, trace=True)
    assert np.isfinite(r["paths"]).all() and (r["paths"] > 0).all()
    _check(model, th, cloud, r, K, N, M, q_steps=(0, H - 1))


def test_terminal_draw_is_uniform_over_the_live_particles():
    """x_next = NULL, H = 1: K M = 4096 draws over 48 live particles of 64.  Each particle's count is binomial
    (4096, 1 / 48): within four standard errors of 4096 / 48, and no dead particle is drawn."""
    model, K, N, M = SU.AR, 64, 64, 64
    rng = np.random.default_rng(5)
    th = _theta(model, K, rng)
    one = _cloud(model, 1, N, 1, rng)
    one[::4] = np.nan
    cloud = np.tile(one, (K, 1, 1))
    r = _smooth(model, th, cloud, M, row0=12345, trace=True)
    counts = np.bincount(r["idx"].reshape(-1), minlength=N)
    live = np.arange(N) % 4 != 0
    n, p = K * M, 1.0 / live.sum()
    se = math.sqrt(n * p * (1.0 - p))
    print(f"counts over the live particles: {counts[live].min()} .. {counts[live].max()}, mean {n * p:.1f}, se {se:.2f}")
    assert counts[~live].sum() == 0 and counts.sum() == n
    assert np.all(np.abs(counts[live] - n * p) <= 4.0 * se)
    assert np.array_equal(r["q"][:, 0], np.broadcast_to(np.where(live, ONE, 0), (K, M, N)))
    _check(model, th, cloud, r, K, N, M, row0=12345, q_steps=(0,))


# ----------------------------------------------------------------------------------------------------------------
# 3. bitwise
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,N,M", [(SU.AR, 1024, 128), (SU.LV, 128, 128), (SU.FHN, 512, 64)])
def test_bitwise_chain_sub_batch_and_repeat(model, N, M):
    K, H = 3, 131
    rng = np.random.default_rng(31 + N)
    th, cloud = _theta(model, K, rng), _cloud(model, K, N, H, rng)
    row0, t0 = 2 ** 32 - N - 5, 11          # the rows cross 2^32
    full = _smooth(model, th, cloud, M, row0=row0, t0=t0)
    _same(full, _smooth(model, th, cloud, M, row0=row0, t0=t0))
    _check(model, th, cloud, full, K, N, M)
    # 131 steps = 64 + 67, the later chunk first, chained through x_first
    b = _smooth(model, th, cloud[:, :, 64:], M, row0=row0, t0=t0 + 64)
    a = _smooth(model, th, cloud[:, :, :64], M, row0=row0, t0=t0, x_next=b["x_first"])
    for k, axis in (("paths", 2), ("idx", 1)):
        assert np.array_equal(_bits(np.concatenate([a[k], b[k]], axis)), _bits(full[k])), k
    assert np.array_equal(_bits(a["x_first"]), _bits(full["x_first"]))
    # no idx asked for: the same paths
    _same(_smooth(model, th, cloud, M, row0=row0, t0=t0, idx=False), full, keys=("paths", "x_first"))
    # each filter alone, at its rows
    for k in range(K):
        sub = _smooth(model, th[k:k + 1], cloud[k * N:(k + 1) * N], M, row0=row0 + k * N, t0=t0)
        for key in ("paths", "x_first", "idx"):
            assert np.array_equal(_bits(sub[key]), _bits(full[key][k * M:(k + 1) * M])), (k, key)
    # fewer trajectories: the first M / 2 of each filter are the same rows, so the same draws
    if M >= 128:
        half = _smooth(model, th, cloud, M // 2, row0=row0, t0=t0)
        for k in range(K):
            assert np.array_equal(_bits(half["paths"][k * M // 2:(k + 1) * M // 2]),
                                  _bits(full["paths"][k * M:k * M + M // 2]))
    for other in (_smooth(model, th, cloud, M, row0=row0 + 1, t0=t0), _smooth(model, th, cloud, M, row0=row0, t0=t0 + 1),
                  _smooth(model, th, cloud, M, row0=row0, t0=t0, seed=SEED + 1)):
        assert not np.array_equal(other["idx"], full["idx"])


def test_refusals():
    from viforssms_amd import _lib, ops
    rng = np.random.default_rng(1)
    g = lambda a: torch.as_tensor(a, device=DEV)
    th, cloud = g(_theta(SU.LV, 2, rng)), g(_cloud(SU.LV, 2, 128, 8, rng))
    call = lambda **kw: ops.particle_smooth(**{**dict(model_id=SU.LV, theta=th, cloud=cloud, dt=0.1, M=64, seed=1,
                                                      row0=0), **kw})
    r = call()
    assert tuple(r.paths.shape) == (128, 2, 8) and r.idx is None and r.q_trace is None
    with pytest.raises(_lib.VissmError, match="SV"):
        call(model_id=SU.SV, theta=g(np.zeros((2, 4), np.float32)))
    with pytest.raises(_lib.VissmError, match="trajectories"):
        call(M=96)
    with pytest.raises(_lib.VissmError, match="trajectories"):
        call(M=256)
    with pytest.raises(_lib.VissmError, match="particles"):
        call(cloud=cloud[:192].contiguous())
    with pytest.raises(_lib.VissmError, match="GPU only"):
        call(theta=th.cpu())
    with pytest.raises(_lib.VissmError, match="cloud"):
        call(cloud=cloud[:, :1].contiguous())
    with pytest.raises(_lib.VissmError, match="horizon"):
        call(cloud=cloud[:, :, :0].contiguous())
    with pytest.raises(_lib.VissmError, match="x_next"):
        call(x_next=torch.zeros(64, 2, device=DEV))


# ----------------------------------------------------------------------------------------------------------------
# 4. statistical
# ----------------------------------------------------------------------------------------------------------------
def test_smoothing_moments_agree_with_the_reference_and_rts():
    """AR, T = 64, obs_std = 1 (tests/golden/pf_ar_series.npz), theta = the generator's, K = 256 filters of N = 256
    particles, M = 64 trajectories each.  Per filter the mean of its M trajectories at each step; then the mean over
    filters and se = the across-filter sd / sqrt(K).  At every step: (a) |mean - mean_ref| <= 4 sqrt(se^2 + se_ref^2)
    against the numpy reference at the same shape; (b) |mean - RTS mean| <= 0.2 smoothing sd; (c) pooled sd / RTS sd
    in [0.85, 1.15].  The reference alone meets them (tests/test_ps_host.py: its largest deviation from RTS is about
    0.1 sd, an O(1 / N) bias of the bootstrap filter); the filter's own means miss (b) by a factor of four."""
    from viforssms_amd import ops
    K, N, M = PS.STAT_K, PS.STAT_N, PS.STAT_M
    obs, obs_bin = PR.stat_case()
    g = lambda a: torch.as_tensor(a, device=DEV)
    th = g(np.tile(np.asarray(SU.TRUE_THETA[SU.AR], np.float32), (K, 1)))
    f = ops.particle_filter(SU.AR, th, g(np.asarray(SU.TRUE_X[SU.AR], np.float32)), g(obs), g(obs_bin), SU.DT[SU.AR],
                            1.0, N, SEED, 123456)
    r = ops.particle_smooth(SU.AR, th, f.cloud, SU.DT[SU.AR], M, SEED ^ 0xABCDEF, 123456)
    paths = r.paths.cpu().numpy().astype(np.float64).reshape(K, M, -1)
    assert np.isfinite(paths).all()
    rts = PS.stat_rts()
    mean, se, sd = PS.stat_moments(paths)
    mean_r, se_r, _ = PS.stat_moments(PS.reference_paths(101))
    bars = PS.stat_bars(mean, se, sd, mean_r, se_r, rts)
    fm = f.cloud.cpu().numpy().astype(np.float64).reshape(K, N, -1).mean((0, 1))
    print(f"(a) share {bars['a'][1]:.3f} (b) {bars['b'][1]:.4f} sd (c) {bars['c'][1][0]:.4f} .. {bars['c'][1][1]:.4f}; "
          f"the filter's means against RTS: {np.max(np.abs(fm - rts['ms']) / np.sqrt(rts['vs'])):.3f} sd")
    assert all(v[0] for v in bars.values()), bars
    assert np.max(np.abs(fm - rts["ms"]) / np.sqrt(rts["vs"])) > 2.0 * PS.MEAN_BAR      # the bars discriminate


# ----------------------------------------------------------------------------------------------------------------
# 5. product
# ----------------------------------------------------------------------------------------------------------------
KF, NF, MF = 8, 128, 64


@pytest.fixture(scope="module", params=["ar", "lv"])
def smoothed(request):
    model = _model(request.param)
    return request.param, model, model.particle_smoother(KF, NF, MF)


def test_product_is_the_filter_plus_the_by_hand_chain(smoothed):
    from viforssms_amd import ops
    from viforssms_amd.summary import column_summary
    from viforssms_amd.vi_ssm import FILTER_SEED_XOR, SMOOTH_SEED_XOR
    family, model, got = smoothed
    _, T, _, S = CASES[family]
    md = model.mdef
    assert sorted(got) == sorted(FILTER_KEYS + SMOOTH_KEYS)
    filt = model.particle_filter(KF, NF)
    for k in FILTER_KEYS:
        assert np.array_equal(_bits(got[k]), _bits(filt[k])), k
    for k, shp in (("smooth/mean", (S, T)), ("smooth/sd", (S, T)), ("smooth/n_valid", (S, T)),
                   ("smooth/quantiles", (5, S, T))):
        assert got[k].shape == shp, k
    assert got["smooth/n_valid"].dtype == np.int64 and got["smooth/n_valid"].max() <= KF * MF
    assert np.isfinite(got["filter/loglik"]).any() and got["smooth/n_valid"].max() > 0, "every filter died"
    th = torch.as_tensor(got["filter/theta"], device=DEV)
    obs, obs_bin, x0 = (torch.as_tensor(a, device=DEV) for a in model.filter_data)
    row0 = model.global_step * KF * NF
    f = ops.particle_filter(md.model_id, th, x0, obs[:, :T].contiguous(), obs_bin[:, :T].contiguous(), md.dt,
                            md.obs_std, NF, model.engine.seed ^ FILTER_SEED_XOR, row0)
    cut = T // 3
    late = ops.particle_smooth(md.model_id, th, f.cloud[:, :, cut:].contiguous(), md.dt, MF,
                               model.engine.seed ^ SMOOTH_SEED_XOR, row0, t0=cut)
    early = ops.particle_smooth(md.model_id, th, f.cloud[:, :, :cut].contiguous(), md.dt, MF,
                                model.engine.seed ^ SMOOTH_SEED_XOR, row0, t0=0, x_next=late.x_first)
    paths = torch.cat([early.paths, late.paths], 2).contiguous()
    s = column_summary(paths.view(KF * MF, S * T), got["probs"], None)
    for k in ("mean", "sd", "n_valid"):
        assert np.array_equal(got[f"smooth/{k}"], s[k].reshape(S, T), equal_nan=True), k
    assert np.array_equal(got["smooth/quantiles"], s["quantiles"].reshape(5, S, T), equal_nan=True)
    # every trajectory of a live filter is made of that filter's particles
    assert np.array_equal(got["smooth/n_valid"], np.isfinite(paths.cpu().numpy()).sum(0))


def test_product_chunking_changes_nothing_and_refusals(smoothed, monkeypatch):
    from viforssms_amd import diagnostics
    family, model, got = smoothed
    for chunk in (7, 64):
        res = model.particle_smoother(KF, NF, MF, chunk=chunk)
        for k in FILTER_KEYS + SMOOTH_KEYS:
            assert np.array_equal(res[k], got[k], equal_nan=True), (chunk, k)
    for bad in (dict(n_paths=96), dict(n_paths=256), dict(n_paths=32), dict(chunk=0), dict(n_particles=100),
                dict(n_theta=model.p_local + 1)):
        with pytest.raises(ValueError):
            model.particle_smoother(**{**dict(n_theta=KF, n_particles=NF, n_paths=MF), **bad})
    _, T, _, S = CASES[family]
    assert diagnostics.SMOOTH_CLOUD_BYTES == 8 << 30
    monkeypatch.setattr(diagnostics, "SMOOTH_CLOUD_BYTES", 4 * KF * NF * S * T - 1)
    with pytest.raises(ValueError, match="lower n_theta or n_particles"):
        model.particle_smoother(KF, NF, MF)
    monkeypatch.setattr(diagnostics, "SMOOTH_CLOUD_BYTES", 4 * KF * NF * S * T)
    res = model.particle_smoother(KF, NF, MF)
    assert np.array_equal(res["smooth/mean"], got["smooth/mean"], equal_nan=True)


def test_product_sv_is_refused_and_save_round_trips(smoothed, tmp_path):
    from tests.parity_util import build_model
    family, model, got = smoothed
    path = str(tmp_path / "sub" / "smooth.npz")
    res = model.save_smoother(path, KF, NF, MF)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(got)
        for k in got:
            assert np.array_equal(z[k], got[k], equal_nan=True) and np.array_equal(res[k], got[k], equal_nan=True), k
    if family == "ar":
        sv = build_model("sv", 7, 40, 8, 2, 16, 5, 3, DEV, T=160, precision=0, seed=3)
        with pytest.raises(ValueError, match="SV"):
            sv.particle_smoother(4, 64, 64)


def test_main_writes_the_smoother(tmp_path, monkeypatch):
    """python main.py hyperparameters.txt ... --smooth 4 64 64 PATH: two training steps, then the .npz."""
    state = np.random.get_state()
    monkeypatch.chdir(tmp_path)          # main.py writes dat/, train/ and model_saves/ under the working directory
    try:
        import main
        out = str(tmp_path / "post" / "smooth.npz")
        model = main.run([os.path.join(ROOT, "hyperparameters.txt"), "-T", "60", "-b", "30", "-k", "5", "-p", "8",
                          "-f", "4", "--steps", "2", "--no-pretrain", "--smooth", "4", "64", "64", out])
    finally:
        np.random.set_state(state)
    assert model.global_step == 2
    with np.load(out) as z:
        assert z["filter/loglik"].shape == (4,) and z["filter/quantiles"].shape == (5, 1, 60)
        assert z["smooth/mean"].shape == (1, 60) and z["smooth/quantiles"].shape == (5, 1, 60)
        # (two steps from a random start leave q(theta) wherever it was drawn: a filter may be dead, its paths NaN)
        assert np.all(z["smooth/n_valid"] <= 4 * 64) and np.all(z["smooth/n_valid"] % 64 == 0)
