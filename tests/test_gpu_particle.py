"""vissm_particle_filter (ops.particle_filter) on the GPU.

Without observations the cloud is bitwise vissm_sde_simulate's output.  With them the kernel is checked teacher-forced,
step by step, against the float64 reference of tests/pf_ref.py applied to the kernel's own previous cloud: the
ancestors exactly (Python-int systematic resampling of the traced integer weights, U from tests/philox_ref.py), the
states within tests/test_gpu_simulate.py's bar 8 * max(e32, 2^-20 * column mean |x|) (e32: the same step in numpy
float32), the weights within the relative error that bar implies for logw, ll_inc and ess against the double formulas
on the traced weights.  Repeated, chunked and sub-batched calls are compared bitwise; degenerate weights, dying
particles and a dead filter end finite, consistent and -inf / NaN; the log-evidence estimates of 256 filters agree
with the reference's and with the exact Kalman value within the bars tests/test_pf_host.py confirms for the reference
alone; VISSMBase.particle_filter equals the by-hand call."""
import math
import os

import numpy as np
import pytest
import torch

from tests import pf_ref as PR
from tests import philox_ref
from tests import sim_util as SU
from tests.parity_util import (FILTER_CASES as CASES, FILTER_KEYS as KEYS, FILTER_KF as KF, FILTER_NF as NF,
                               filter_model as _model)
from tests.sim_util import (PF_OBS_STD as OBS_STD, PF_ONE as ONE, PF_SEED as SEED, filter_inputs as _inputs,
                            filter_series as _series, resample_u as _resample_u, same_bits as _same, state_bar as _bar,
                            bits as _bits)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(model, th, x0, obs, obs_bin, N, row0=0, t0=0, H=None, loglik_in=None, cloud=True, trace=True, seed=SEED):
    from viforssms_amd import ops
    g = lambda a: torch.as_tensor(a, device=DEV)
    r = ops.particle_filter(model, g(th), g(x0), g(obs), g(obs_bin), SU.DT[model], OBS_STD[model], N, seed, row0,
                            t0=t0, loglik_in=None if loglik_in is None else g(loglik_in), cloud=cloud, trace=trace,
                            H=H)
    torch.cuda.synchronize()
    c = lambda t: None if t is None else t.cpu().numpy()
    return {"loglik": c(r.loglik), "ll_inc": c(r.ll_inc), "ess": c(r.ess), "state_end": c(r.state_end),
            "cloud": c(r.cloud), "q": c(r.q_trace), "anc": c(r.anc_trace)}


def _logw32(x, y, b, sd):
    """pf_ref.obs_logw in numpy float32 arithmetic: what fp32 costs the log-weight."""
    f = np.float32
    lw = np.zeros(x.shape[:-1], f)
    for d in range(x.shape[-1]):
        if b[d] != 0:
            z = (x[..., d].astype(f) - f(y[d])) / f(sd)
            lw = lw + f(b[d]) * (f(-0.5) * z * z - np.log(f(sd)) - f(PR.HALF_LOG_2PI))
    return lw


# ----------------------------------------------------------------------------------------------------------------
# 1. no observations: the forecast kernel's paths
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,K,N,H", [(SU.AR, 1, 64, 1), (SU.AR, 3, 128, 63), (SU.AR, 5, 1024, 131),
                                         (SU.LV, 5, 1024, 64), (SU.LV, 1, 128, 131), (SU.FHN, 3, 64, 65),
                                         (SU.FHN, 3, 1024, 65)])
def test_without_observations_the_cloud_is_the_forecast(model, K, N, H):
    from viforssms_amd import ops
    rng = np.random.default_rng(100 * model + K + N + H)
    th, x0 = _inputs(model, K, N, rng)
    obs, obs_bin = _series(model, H, "none", rng)
    row0 = 5 + 1000 * K
    r = _run(model, th, x0, obs, obs_bin, N, row0=row0)
    x, _, xe = ops.sde_simulate(model, torch.as_tensor(np.repeat(th, N, 0), device=DEV),
                                torch.as_tensor(x0, device=DEV), H, SU.DT[model], SEED, row0)
    assert r["cloud"].shape == (K * N, SU.S_OF[model], H)
    assert np.array_equal(_bits(r["cloud"]), _bits(x.cpu().numpy()))
    assert np.array_equal(_bits(r["state_end"]), _bits(xe.cpu().numpy()))
    assert np.array_equal(r["loglik"], np.zeros(K)) and np.array_equal(r["ll_inc"], np.zeros((K, H), np.float32))
    assert np.array_equal(r["ess"], np.full((K, H), N, np.float32))
    assert not r["q"].any() and np.array_equal(r["anc"], np.broadcast_to(np.arange(N, dtype=np.int32), (K, H, N)))


# ----------------------------------------------------------------------------------------------------------------
# 2. teacher-forced parity
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,pattern,K,N,H", [
    (SU.AR, "all", 3, 64, 65), (SU.AR, "tenth", 1, 1024, 131), (SU.AR, "all", 5, 128, 1),
    (SU.LV, "all", 3, 128, 64), (SU.LV, "coord", 5, 64, 63), (SU.LV, "tenth", 1, 1024, 65),
    (SU.FHN, "all", 1, 128, 131), (SU.FHN, "coord", 3, 64, 65), (SU.FHN, "tenth", 3, 1024, 63),
    (SU.FHN, "all", 5, 1024, 1),
    # four and eight waves (two and four trips of the partial-sum loop), one tile boundary each
    (SU.AR, "tenth", 3, 256, 65), (SU.AR, "coord", 3, 512, 65), (SU.LV, "coord", 3, 256, 65),
    (SU.LV, "coord", 3, 512, 33), (SU.FHN, "tenth", 3, 256, 65), (SU.FHN, "coord", 3, 512, 33)])
def test_teacher_forced_parity(model, pattern, K, N, H):
    """Step t of the reference starts from the kernel's own cloud at t - 1, so rounding does not compound and a
    resampling decision of the kernel is never second-guessed: given its traced weights its ancestors must be the
    Python-int ones exactly.

    Weights: the kernel's logw_i and m each lie within d = 8 * max(e32, 2^-20 mean |logw|) of the float64 ones (e32:
    numpy float32 against float64, propagated state and density), so exp(logw_i - m) is off by a factor within
    e^(2 d); the fp32 rounding of the difference and of the exp add (|logw_i - m| + 2) 2^-23 relative, the
    truncation one unit."""
    from viforssms_amd import ops
    S, P, dt, sd = SU.S_OF[model], SU.P_OF[model], SU.DT[model], OBS_STD[model]
    rng = np.random.default_rng(1000 * model + 10 * N + H + K)
    th, x0 = _inputs(model, K, N, rng)
    obs, obs_bin = _series(model, H, pattern, rng)
    row0 = 3 + 7 * N
    r = _run(model, th, x0, obs, obs_bin, N, row0=row0)
    eps, _ = ops.normal_base(SEED, row0, K * N, S * H, 0, DEV)
    nn = eps.cpu().numpy().reshape(K * N, H, S)
    th_rows = np.repeat(th, N, 0)
    cloud, anc, q = r["cloud"], r["anc"].astype(np.int64), r["q"]
    assert np.isfinite(cloud).all(), "the stable-range inputs left the domain"
    exp64, exp32 = np.empty((K * N, S, H)), np.empty((K * N, S, H), np.float32)
    prev = x0
    shares = {"q": 0.0, "ll_inc": 0.0, "ess": 0.0}
    ll_sum, ll_bar = np.zeros(K), np.zeros(K)
    n_obs = 0
    for t in range(H):
        p64 = SU.step(model, prev.astype(np.float64), th_rows.astype(np.float64), dt, nn[:, t].astype(np.float64))
        p32 = SU.step(model, prev.astype(np.float32), th_rows, dt, nn[:, t])
        assert SU.alive(model, p64).all() and p32.dtype == np.float32
        rows = (np.arange(K)[:, None] * N + anc[:, t, :]).reshape(-1)
        exp64[:, :, t], exp32[:, :, t] = p64[rows], p32[rows]
        prev = cloud[:, :, t]
        if not np.any(obs_bin[:, t] != 0):
            assert not q[:, t].any() and np.array_equal(anc[:, t], np.broadcast_to(np.arange(N), (K, N)))
            assert np.all(r["ll_inc"][:, t] == 0.0) and np.all(r["ess"][:, t] == float(N))
            continue
        n_obs += 1
        for k in range(K):
            sl = slice(k * N, (k + 1) * N)
            alive, lw64, m64, qref = PR.weigh(model, p64[sl], obs[:, t], obs_bin[:, t], sd)
            lw32 = _logw32(p32[sl], obs[:, t], obs_bin[:, t], sd)
            qk = [int(v) for v in q[k, t]]
            want_anc, W = PR.systematic_ints(qk, _resample_u(SEED, t, row0 + k * N))
            assert W > 0 and max(qk) == ONE
            assert anc[k, t].tolist() == want_anc, (k, t)
            d = 8.0 * max(float(np.max(np.abs(lw32 - lw64))), 2.0 ** -20 * float(np.mean(np.abs(lw64))))
            qr = qref.astype(np.float64)
            tol = qr * (math.expm1(2.0 * d) + (np.abs(lw64 - m64) + 2.0) * 2.0 ** -23) + 1.0
            err = np.abs(np.asarray(qk, np.float64) - qr)
            assert np.all(err <= tol), (k, t, float(np.max(err / tol)))
            shares["q"] = max(shares["q"], float(np.max(err / tol)))
            v = PR.ll_increment(m64, W, N)
            # (the error of a maximum is at most the largest error of its entries)
            bar = 8.0 * max(float(np.max(np.abs(lw32 - lw64))), 2.0 ** -20 * abs(v))
            assert abs(float(r["ll_inc"][k, t]) - v) <= bar, (k, t)
            shares["ll_inc"] = max(shares["ll_inc"], abs(float(r["ll_inc"][k, t]) - v) / bar)
            ll_sum[k] += v
            ll_bar[k] += bar
            e = PR.ess(qk)
            assert abs(float(r["ess"][k, t]) - e) <= 8.0 * 2.0 ** -20 * e, (k, t)
            shares["ess"] = max(shares["ess"], abs(float(r["ess"][k, t]) - e) / (8.0 * 2.0 ** -20 * e))
            assert 1.0 <= e <= N
    assert n_obs == int(np.any(obs_bin != 0, axis=0).sum())
    bar, e32 = _bar(exp64, exp32)
    dev = np.abs(cloud - exp64)
    print(f"model {model} {pattern} K {K} N {N} H {H}: e32 {e32:.3e}, shares of the bars: cloud "
          f"{np.max(dev / bar):.3f} q {shares['q']:.3f} ll_inc {shares['ll_inc']:.3f} ess {shares['ess']:.3f}")
    assert np.all(dev <= bar)
    assert np.all(np.abs(r["loglik"] - ll_sum) <= ll_bar + 1e-12)
    assert np.array_equal(_bits(r["state_end"]), _bits(cloud[:, :, -1]))


# ----------------------------------------------------------------------------------------------------------------
# 3. bitwise
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,pattern,N", [(SU.LV, "tenth", 128), (SU.AR, "all", 1024), (SU.FHN, "coord", 64)])
def test_bitwise_repeat_chunks_and_sub_batch(model, pattern, N):
    K, H = 5, 131
    rng = np.random.default_rng(31 + N)
    th, x0 = _inputs(model, K, N, rng)
    obs, obs_bin = _series(model, H, pattern, rng)
    row0 = 2 ** 32 - 3 * N          # the rows cross 2^32
    full = _run(model, th, x0, obs, obs_bin, N, row0=row0)
    _same(full, _run(model, th, x0, obs, obs_bin, N, row0=row0))
    assert np.isfinite(full["loglik"]).all() and (full["q"] > 0).any()
    # 131 steps = 50 + 81 chained through state_end and loglik (the first call sees only its own 50 observations)
    a = _run(model, th, x0, obs[:, :50], obs_bin[:, :50], N, row0=row0)
    b = _run(model, th, a["state_end"], obs, obs_bin, N, row0=row0, t0=50, loglik_in=a["loglik"])
    assert b["cloud"].shape[2] == 81
    for k, axis in (("ll_inc", 1), ("ess", 1), ("cloud", 2), ("q", 1), ("anc", 1)):
        assert np.array_equal(_bits(np.concatenate([a[k], b[k]], axis)), _bits(full[k])), k
    _same(b, full, keys=("loglik", "state_end"))
    # cloud = NULL and no trace: the same numbers
    _same(_run(model, th, x0, obs, obs_bin, N, row0=row0, cloud=False, trace=False), full,
          keys=("loglik", "ll_inc", "ess", "state_end"))
    # filters 2 .. 4 alone, at their rows
    sub = _run(model, th[2:], x0[2 * N:], obs, obs_bin, N, row0=row0 + 2 * N)
    for k in ("loglik", "ll_inc", "ess", "q", "anc"):
        assert np.array_equal(_bits(sub[k]), _bits(full[k][2:])), k
    for k in ("state_end", "cloud"):
        assert np.array_equal(_bits(sub[k]), _bits(full[k][2 * N:])), k
    other = _run(model, th, x0, obs, obs_bin, N, row0=row0 + 1)
    assert not np.array_equal(other["cloud"], full["cloud"])


# ----------------------------------------------------------------------------------------------------------------
# 4. degenerate and dead
# ----------------------------------------------------------------------------------------------------------------
def test_observation_forty_sd_away_stays_finite():
    model, K, N, H = SU.AR, 3, 64, 4
    rng = np.random.default_rng(41)
    th, x0 = _inputs(model, K, N, rng)
    obs, obs_bin = _series(model, H, "none", rng)
    free = _run(model, th, x0, obs, obs_bin, N)
    obs[0, 1] = free["cloud"][:, 0, 1].max() + 40.0 * OBS_STD[model]
    obs_bin[0, 1] = 1.0
    r = _run(model, th, x0, obs, obs_bin, N)
    assert np.array_equal(_bits(r["cloud"][:, :, 0]), _bits(free["cloud"][:, :, 0]))
    assert np.isfinite(r["loglik"]).all() and np.isfinite(r["cloud"]).all() and np.isfinite(r["ess"]).all()
    assert np.all(r["q"][:, 1].max(1) == ONE) and np.all(r["ll_inc"][:, 1] <= -0.5 * 40.0 ** 2)
    assert np.array_equal(r["loglik"], r["ll_inc"][:, 1].astype(np.float64)) or \
        np.all(np.abs(r["loglik"] - r["ll_inc"][:, 1]) <= 2.0 ** -20 * np.abs(r["loglik"]))
    for k in range(K):
        want, _ = PR.systematic_ints(r["q"][k, 1], _resample_u(SEED, 1, k * N))
        assert r["anc"][k, 1].tolist() == want


def test_dying_particles_get_no_weight():
    """LV started next to the boundary (tests/test_gpu_simulate.py's dead-row case): particles leave the positive
    orthant between observations.  A particle whose previous state is NaN has q = 0; no ancestor has q = 0; after a
    resampling every slot is alive again; n_valid of the column summary is the count of finite rows."""
    from viforssms_amd.summary import column_summary
    model, K, N, H = SU.LV, 3, 128, 40
    rng = np.random.default_rng(12)
    th = np.tile(np.asarray(SU.TRUE_THETA[model], np.float32), (K, 1))
    x0 = np.stack([rng.uniform(0.1, 1.5, K * N), np.full(K * N, 100.0)], 1).astype(np.float32)
    obs = -np.ones((2, H), np.float32)
    obs_bin = np.zeros((2, H), np.float32)
    free = _run(model, th, x0, obs, obs_bin, N)
    dead_free = np.isnan(free["cloud"][:, 0, :])
    assert 0.10 <= dead_free[:, -1].mean() <= 0.90, dead_free[:, -1].mean()
    steps = np.arange(7, H, 8)
    obs_bin[1, steps] = 1.0
    obs[1, steps] = np.nanmedian(free["cloud"][:, 1, steps], axis=0) + rng.standard_normal(steps.size)
    r = _run(model, th, x0, obs, obs_bin, N)
    cloud, q, anc = r["cloud"], r["q"], r["anc"]
    nan = np.isnan(cloud)
    assert np.array_equal(nan[:, 0], nan[:, 1]) and np.isfinite(r["loglik"]).all()
    died = 0
    for t in steps:
        before = nan[:, 0, t - 1].reshape(K, N)
        died += int(before.sum())
        assert not q[:, t][before].any()                                  # dead before the step: no weight
        assert np.all(np.take_along_axis(q[:, t], anc[:, t].astype(np.int64), 1) > 0)    # never an ancestor
        assert not nan[:, :, t].any()                                     # every slot alive after the resampling
        assert np.all(r["ess"][:, t] >= 1.0) and np.all(r["ess"][:, t] <= N - before.sum(1))
    assert died > 0, "no particle died before an observation: nothing was checked"
    for t in range(1, H):
        if t not in steps:
            assert np.all(nan[:, 0, t] >= nan[:, 0, t - 1])               # between observations the dead stay dead
    s = column_summary(torch.as_tensor(cloud.reshape(K * N, 2 * H), device=DEV))
    assert np.array_equal(s["n_valid"], np.isfinite(cloud).sum(0).reshape(-1))
    assert s["n_valid"].min() < K * N and s["n_valid"].max() == K * N


def test_dead_filter_finishes():
    """Filter 1 of 3 starts with every particle outside the domain: -inf, NaN throughout, and its neighbours are the
    filters they are without it; chained, it stays dead."""
    model, K, N, H = SU.LV, 3, 64, 70
    rng = np.random.default_rng(43)
    th, x0 = _inputs(model, K, N, rng)
    obs, obs_bin = _series(model, H, "tenth", rng)
    good = _run(model, th, x0, obs, obs_bin, N)
    bad0 = x0.copy()
    bad0[N:2 * N, 0] = np.where(np.arange(N) % 2 == 0, -1.0, np.nan)
    r = _run(model, th, bad0, obs, obs_bin, N)
    assert r["loglik"][1] == -np.inf and np.isfinite(r["loglik"][[0, 2]]).all()
    first = 9
    assert np.isnan(r["cloud"][N:2 * N]).all() and np.isnan(r["state_end"][N:2 * N]).all()
    assert np.isnan(r["ll_inc"][1, first:]).all() and np.isnan(r["ess"][1, first:]).all()
    assert np.all(r["ll_inc"][1, :first] == 0.0) and np.all(r["ess"][1, :first] == N)   # nothing observed yet
    assert not r["q"][1].any() and np.array_equal(r["anc"][1], np.broadcast_to(np.arange(N), (H, N)))
    for k in (0, 2):
        for key in ("ll_inc", "ess", "q", "anc"):
            assert np.array_equal(_bits(r[key][k]), _bits(good[key][k])), (k, key)
        assert np.array_equal(_bits(r["cloud"][k * N:(k + 1) * N]), _bits(good["cloud"][k * N:(k + 1) * N]))
    a = _run(model, th, bad0, obs[:, :30], obs_bin[:, :30], N)
    b = _run(model, th, a["state_end"], obs, obs_bin, N, t0=30, loglik_in=a["loglik"])
    assert b["loglik"][1] == -np.inf and np.isnan(b["ll_inc"][1]).all() and np.isnan(b["ess"][1]).all()
    _same(b, r, keys=("loglik", "state_end"))
    assert np.array_equal(_bits(np.concatenate([a["cloud"], b["cloud"]], 2)), _bits(r["cloud"]))
    assert np.array_equal(_bits(np.concatenate([a["ll_inc"], b["ll_inc"]], 1)), _bits(r["ll_inc"]))


def test_refusals():
    from viforssms_amd import _lib, ops
    th, x0 = _inputs(SU.LV, 2, 64, np.random.default_rng(1))
    g = lambda a: torch.as_tensor(a, device=DEV)
    obs, b = g(np.zeros((2, 8), np.float32)), g(np.zeros((2, 8), np.float32))
    call = lambda **kw: ops.particle_filter(**{**dict(model_id=SU.LV, theta=g(th), x_start=g(x0), obs=obs, obs_bin=b,
                                                      dt=0.1, obs_std=1.0, N=64, seed=1, row0=0), **kw})
    r = call(H=0)
    assert tuple(r.cloud.shape) == (128, 2, 0) and torch.equal(r.state_end, g(x0)) and not r.loglik.any()
    r = call(x_start=g(x0[0]))
    assert tuple(r.cloud.shape) == (128, 2, 8)
    with pytest.raises(_lib.VissmError, match="SV"):
        call(model_id=SU.SV, theta=g(np.zeros((2, 4), np.float32)))
    with pytest.raises(_lib.VissmError, match="particles"):
        call(N=96)
    with pytest.raises(_lib.VissmError, match="GPU only"):
        call(theta=torch.as_tensor(th))
    with pytest.raises(_lib.VissmError, match="x_start"):
        call(x_start=g(x0[:64]))
    with pytest.raises(_lib.VissmError, match="obs"):
        call(obs_bin=b[:, :4].contiguous())
    with pytest.raises(_lib.VissmError, match="horizon"):
        call(t0=5, H=4)
    with pytest.raises(_lib.VissmError, match="loglik_in"):
        call(loglik_in=torch.zeros(2, device=DEV))


# ----------------------------------------------------------------------------------------------------------------
# 5. statistical
# ----------------------------------------------------------------------------------------------------------------
def test_log_evidence_agrees_with_the_reference_and_kalman():
    """AR, T = 64, N = 256, K = 256 filters at the generator's theta, obs_std = 1, about 70 % of the steps observed
    (tests/golden/pf_ar_series.npz).  mu, s: the kernel's mean and sd of loglik; mu_r, s_r: the reference's over
    K_r = 1024 free-running filters; L: the exact Kalman value; se = sqrt(s^2 / K + s_r^2 / K_r).
    |mu - mu_r| <= 4 se; s / s_r in [0.8, 1.25]; -4 se <= L - mu <= s_r^2 + 4 se (pf_ref.stat_bars)."""
    K, N = 256, 256
    obs, obs_bin = PR.stat_case()
    th = np.tile(np.asarray(SU.TRUE_THETA[SU.AR], np.float32), (K, 1))
    x0 = np.asarray(SU.TRUE_X[SU.AR], np.float32)
    r = _run(SU.AR, th, x0, obs, obs_bin, N, row0=123456, trace=False, cloud=False)
    ll = r["loglik"]
    assert np.isfinite(ll).all()
    ref = PR.reference_logliks(101)
    L = PR.stat_kalman()
    mu, s, mu_r, s_r = ll.mean(), ll.std(ddof=1), ref.mean(), ref.std(ddof=1)
    bars = PR.stat_bars(mu, s, K, mu_r, s_r, ref.size, L)
    print(f"L {L:.4f} mu {mu:.4f} s {s:.4f} mu_r {mu_r:.4f} s_r {s_r:.4f} L - mu {L - mu:.4f} {bars}")
    assert all(bars.values()), bars
    assert np.all(np.abs(r["ll_inc"].astype(np.float64).sum(1) - ll) <= 64 * 2.0 ** -20 * np.abs(ll))
    assert np.all(r["ess"][:, obs_bin[0] == 0] == N) and np.all(r["ess"] >= 1.0) and np.all(r["ess"] <= N)


# ----------------------------------------------------------------------------------------------------------------
# 6. product
# ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["ar", "lv"])
def filtered(request):
    model = _model(request.param)
    return request.param, model, model.particle_filter(KF, NF)


def test_product_keys_shapes_and_by_hand_call(filtered):
    from viforssms_amd import ops
    from viforssms_amd.vi_ssm import FILTER_SEED_XOR
    family, model, got = filtered
    _, T, _, S = CASES[family]
    md = model.mdef
    assert sorted(got) == sorted(KEYS)
    P = SU.P_OF[md.model_id]
    shapes = {"probs": (5,), "filter/loglik": (KF,), "filter/theta": (KF, P), "filter/ll_inc": (KF, T),
              "filter/ess": (KF, T), "filter/mean": (S, T), "filter/sd": (S, T), "filter/n_valid": (S, T),
              "filter/quantiles": (5, S, T)}
    for k, shp in shapes.items():
        assert got[k].shape == shp, k
    assert got["filter/loglik"].dtype == np.float64 and got["filter/n_valid"].dtype == np.int64
    _, theta = model.sample_paths_theta(np.tile(0, model.p_local), step=model.global_step)
    th = theta.detach().float()[:KF].contiguous()
    assert np.array_equal(got["filter/theta"], th.cpu().numpy())
    obs, obs_bin, x0 = (torch.as_tensor(a, device=DEV) for a in model.filter_data)
    r = ops.particle_filter(md.model_id, th, x0, obs[:, :T].contiguous(), obs_bin[:, :T].contiguous(), md.dt,
                            md.obs_std, NF, model.engine.seed ^ FILTER_SEED_XOR, model.global_step * KF * NF)
    assert np.array_equal(_bits(got["filter/loglik"]), _bits(r.loglik.cpu().numpy()))
    assert np.array_equal(_bits(got["filter/ll_inc"]), _bits(r.ll_inc.cpu().numpy()))
    assert np.isfinite(got["filter/loglik"]).any(), "every filter died: nothing is compared"
    c64 = r.cloud.cpu().numpy().astype(np.float64)
    assert np.array_equal(got["filter/n_valid"], np.isfinite(c64).sum(0))
    some = got["filter/n_valid"] > 0
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        rq = np.nanquantile(c64, got["probs"], axis=0)
    assert np.allclose(got["filter/quantiles"][:, some], rq[:, some], rtol=1e-12, atol=0.0)
    assert (got["filter/ll_inc"][:, (model.filter_data[1][:, :T] == 0).all(0)] == 0).all()


def test_product_chunking_changes_nothing(filtered):
    family, model, got = filtered
    for chunk in (7, 64):
        res = model.particle_filter(KF, NF, chunk=chunk)
        for k in KEYS:
            assert np.array_equal(res[k], got[k], equal_nan=True), (chunk, k)
    assert model.filter_chunk(64, 1024) % 64 == 0 and model.filter_chunk(10 ** 6, 1024) == 64
    with pytest.raises(ValueError):
        model.particle_filter(KF, NF, chunk=0)
    with pytest.raises(ValueError):
        model.particle_filter(model.p_local + 1, NF)
    with pytest.raises(ValueError):
        model.particle_filter(KF, 100)


def test_product_sv_is_refused_and_save_round_trips(filtered, tmp_path):
    from tests.parity_util import build_model
    family, model, got = filtered
    path = str(tmp_path / "sub" / "filter.npz")
    res = model.save_filter(path, KF, NF)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(got)
        for k in got:
            assert np.array_equal(z[k], got[k], equal_nan=True) and np.array_equal(res[k], got[k], equal_nan=True), k
    if family == "ar":
        sv = build_model("sv", 7, 40, 8, 2, 16, 5, 3, DEV, T=160, precision=0, seed=3)
        with pytest.raises(ValueError, match="SV"):
            sv.particle_filter(4, 64)


def test_main_writes_the_filter(tmp_path, monkeypatch):
    """python main.py hyperparameters.txt ... --filter 4 64 PATH: two training steps, then the .npz."""
    state = np.random.get_state()
    monkeypatch.chdir(tmp_path)          # main.py writes dat/, train/ and model_saves/ under the working directory
    try:
        import main
        out = str(tmp_path / "post" / "filter.npz")
        model = main.run([os.path.join(ROOT, "hyperparameters.txt"), "-T", "60", "-b", "30", "-k", "5", "-p", "8",
                          "-f", "4", "--steps", "2", "--no-pretrain", "--filter", "4", "64", out])
    finally:
        np.random.set_state(state)
    assert model.global_step == 2
    with np.load(out) as z:
        assert z["filter/loglik"].shape == (4,) and z["filter/quantiles"].shape == (5, 1, 60)
        # (two steps from a random start leave q(theta) wherever it was drawn: a filter may be dead, NaN)
        assert z["filter/ess"].shape == (4, 60) and np.all((z["filter/ess"] <= 64) | np.isnan(z["filter/ess"]))
        assert z["filter/theta"].shape == (4, 3) and np.all(z["filter/n_valid"] <= 4 * 64)
