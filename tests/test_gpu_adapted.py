"""vissm_particle_filter_adapted (ops.particle_filter(proposal="adapted")) on the GPU.

Without observations every output is bitwise vissm_particle_filter's, hence the forecast's.  With them the kernel is
checked teacher-forced, step by step, against the float64 reference of tests/gpf_ref.py (numpy.linalg on the general
formulas) applied to the kernel's own previous cloud: the weights of the *pre-step* states within the q bar of
tests/test_gpu_particle.py, the ancestors exactly (Python-int systematic resampling of the traced weights), the new
states within 8 * max(e32, 2^-20 * column mean |x|) of the float64 conditional draw from the ancestor's state with
the slot's own normals.  Repeated, chunked and sub-batched calls are compared bitwise; a far observation, dying LV
particles and a dead filter end finite, consistent and -inf / NaN; the log-evidence estimates agree with the adapted
reference's and with Kalman and are at least four times tighter than the bootstrap reference's; the smoother runs on
the adapted cloud; the product path carries the keyword through."""
import math
import os

import numpy as np
import pytest
import torch

from tests import gpf_ref as GR
from tests import pf_ref as PR
from tests import ps_ref as PS
from tests import sim_util as SU
from tests.parity_util import (FILTER_CASES as CASES, FILTER_KEYS as KEYS, FILTER_KF as KF, FILTER_NF as NF,
                               filter_model as _model)
from tests.sim_util import (PF_OBS_STD as OBS_STD, PF_ONE as ONE, PF_SEED as SEED, filter_inputs as _inputs,
                            filter_series as _series, resample_u as _resample_u, same_bits as _same, state_bar as _bar,
                            bits as _bits)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(model, th, x0, obs, obs_bin, N, row0=0, t0=0, H=None, loglik_in=None, cloud=True, trace=True, seed=SEED,
         proposal="adapted", obs_std=None):
    from viforssms_amd import ops
    g = lambda a: torch.as_tensor(a, device=DEV)
    r = ops.particle_filter(model, g(th), g(x0), g(obs), g(obs_bin), SU.DT[model],
                            OBS_STD[model] if obs_std is None else obs_std, N, seed, row0, t0=t0,
                            loglik_in=None if loglik_in is None else g(loglik_in), cloud=cloud, trace=trace, H=H,
                            proposal=proposal)
    torch.cuda.synchronize()
    c = lambda t: None if t is None else t.cpu().numpy()
    return {"loglik": c(r.loglik), "ll_inc": c(r.ll_inc), "ess": c(r.ess), "state_end": c(r.state_end),
            "cloud": c(r.cloud), "q": c(r.q_trace), "anc": c(r.anc_trace)}


def _eq(a, b):
    """array_equal with NaN == NaN for the float entries (the proposal's name is a string array)."""
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _masked(model, H, pattern, rng):
    """tests/test_gpu_particle.py's series observed everywhere, then masked -- "all": every coordinate at every step;
    "tenth": every coordinate at steps 9, 19, .. and at the first and the last step; "first": coordinate 0 only, at
    steps 0, 3, ..; "second": coordinate 1 only, at steps 1, 4, .. and the last.  Unobserved entries hold -1."""
    y, _ = _series(model, H, "all", rng)
    S = SU.S_OF[model]
    b = np.zeros((S, H), np.float32)
    if pattern == "all":
        b[:] = 1.0
    elif pattern == "tenth":
        b[:, 9::10] = 1.0
        b[:, 0] = b[:, H - 1] = 1.0
    elif pattern == "first":
        b[0, 0::3] = 1.0
    elif pattern == "second":
        b[S - 1, 1::3] = 1.0
        b[S - 1, H - 1] = 1.0
    return np.where(b > 0, y, np.float32(-1.0)).astype(np.float32), b


# ----------------------------------------------------------------------------------------------------------------
# 1. no observations: the bootstrap kernel's bits, hence the forecast's
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,K,N,H", [(SU.AR, 1, 64, 1), (SU.LV, 3, 128, 63), (SU.FHN, 5, 1024, 131)])
def test_without_observations_it_is_the_bootstrap_filter(model, K, N, H):
    from viforssms_amd import ops
    rng = np.random.default_rng(100 * model + K + N + H)
    th, x0 = _inputs(model, K, N, rng)
    obs, obs_bin = _series(model, H, "none", rng)
    row0 = 5 + 1000 * K
    r = _run(model, th, x0, obs, obs_bin, N, row0=row0)
    _same(r, _run(model, th, x0, obs, obs_bin, N, row0=row0, proposal="bootstrap"))
    x, _, xe = ops.sde_simulate(model, torch.as_tensor(np.repeat(th, N, 0), device=DEV),
                                torch.as_tensor(x0, device=DEV), H, SU.DT[model], SEED, row0)
    assert np.array_equal(_bits(r["cloud"]), _bits(x.cpu().numpy()))
    assert np.array_equal(_bits(r["state_end"]), _bits(xe.cpu().numpy()))
    assert np.array_equal(r["loglik"], np.zeros(K)) and not r["q"].any()


# ----------------------------------------------------------------------------------------------------------------
# 2. teacher-forced parity
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,pattern,K,N,H", [
    (SU.AR, "all", 3, 64, 65), (SU.AR, "tenth", 1, 1024, 131), (SU.AR, "all", 3, 128, 1),
    (SU.LV, "all", 3, 128, 64), (SU.LV, "first", 3, 64, 63), (SU.LV, "second", 1, 1024, 65),
    (SU.LV, "tenth", 1, 128, 131), (SU.FHN, "all", 1, 128, 131), (SU.FHN, "second", 3, 64, 65),
    (SU.FHN, "first", 3, 1024, 63), (SU.FHN, "all", 3, 1024, 1),
    # four and eight waves (two and four trips of the partial-sum loop), one tile boundary each
    (SU.AR, "tenth", 3, 256, 65), (SU.AR, "first", 3, 512, 65), (SU.LV, "second", 3, 256, 65),
    (SU.LV, "first", 3, 512, 33), (SU.FHN, "tenth", 3, 256, 65), (SU.FHN, "second", 3, 512, 33)])
def test_teacher_forced_parity(model, pattern, K, N, H):
    """Step t of the reference starts from the kernel's own cloud at t - 1 (x_start at t = 0).  At an observed step
    the weights are those of that *pre-step* cloud: the kernel's logw_i and m each lie within d = 8 * max(e32, 2^-20
    mean |logw|) of the float64 ones, so q is held to tests/test_gpu_particle.py's q bar; given its traced weights
    the ancestors must be the Python-int ones exactly; slot j's new state is the conditional draw from ancestor
    anc[j]'s pre-step state with the slot's own normals."""
    from viforssms_amd import ops
    S, dt, sd = SU.S_OF[model], SU.DT[model], OBS_STD[model]
    rng = np.random.default_rng(2000 * model + 10 * N + H + K)
    th, x0 = _inputs(model, K, N, rng)
    obs, obs_bin = _masked(model, H, pattern, rng)
    row0 = 3 + 7 * N
    r = _run(model, th, x0, obs, obs_bin, N, row0=row0)
    eps, _ = ops.normal_base(SEED, row0, K * N, S * H, 0, DEV)
    nn = eps.cpu().numpy().reshape(K * N, H, S)
    th_rows = np.repeat(th, N, 0)
    th64 = th_rows.astype(np.float64)
    cloud, anc, q = r["cloud"], r["anc"].astype(np.int64), r["q"]
    assert np.isfinite(cloud).all(), "the stable-range inputs left the domain"
    exp64, exp32 = np.empty((K * N, S, H)), np.empty((K * N, S, H), np.float32)
    prev = x0
    shares = {"q": 0.0, "ll_inc": 0.0, "ess": 0.0}
    ll_sum, ll_bar = np.zeros(K), np.zeros(K)
    n_obs = 0
    for t in range(H):
        y, b = obs[:, t], obs_bin[:, t]
        if not np.any(b != 0):
            exp64[:, :, t] = SU.step(model, prev.astype(np.float64), th64, dt, nn[:, t].astype(np.float64))
            exp32[:, :, t] = SU.step(model, prev.astype(np.float32), th_rows, dt, nn[:, t])
            assert not q[:, t].any() and np.array_equal(anc[:, t], np.broadcast_to(np.arange(N), (K, N)))
            assert np.all(r["ll_inc"][:, t] == 0.0) and np.all(r["ess"][:, t] == float(N))
            prev = cloud[:, :, t]
            continue
        n_obs += 1
        mu32, Sg32 = GR.moments(model, prev.astype(np.float32), th_rows, dt)
        lw32_all = GR.predictive_logw(mu32, Sg32, y, b, np.float32(sd)).astype(np.float64)
        for k in range(K):
            sl = slice(k * N, (k + 1) * N)
            alive, lw64, m64, qref = GR.weigh(model, prev[sl].astype(np.float64), th64[sl], dt, y, b, sd)
            assert alive.all()
            lw32 = lw32_all[sl]
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
            bar = 8.0 * max(float(np.max(np.abs(lw32 - lw64))), 2.0 ** -20 * abs(v))
            assert abs(float(r["ll_inc"][k, t]) - v) <= bar, (k, t)
            shares["ll_inc"] = max(shares["ll_inc"], abs(float(r["ll_inc"][k, t]) - v) / bar)
            ll_sum[k] += v
            ll_bar[k] += bar
            e = PR.ess(qk)
            assert abs(float(r["ess"][k, t]) - e) <= 8.0 * 2.0 ** -20 * e, (k, t)
            shares["ess"] = max(shares["ess"], abs(float(r["ess"][k, t]) - e) / (8.0 * 2.0 ** -20 * e))
            assert 1.0 <= e <= N
        rows = (np.arange(K)[:, None] * N + anc[:, t, :]).reshape(-1)
        xa = prev[rows]
        exp64[:, :, t] = GR.propagate(model, xa.astype(np.float64), th64, dt, y, b, sd, nn[:, t].astype(np.float64))
        exp32[:, :, t] = GR.propagate(model, xa.astype(np.float32), th_rows, dt, y, b, np.float32(sd), nn[:, t])
        prev = cloud[:, :, t]
    assert n_obs == int(np.any(obs_bin != 0, axis=0).sum()) and n_obs > 0
    assert SU.alive(model, exp64.transpose(0, 2, 1)).all()
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
@pytest.mark.parametrize("model,pattern,N", [(SU.LV, "tenth", 128), (SU.AR, "all", 1024), (SU.FHN, "first", 64)])
def test_bitwise_repeat_chunks_and_sub_batch(model, pattern, N):
    K, H = 5, 131
    rng = np.random.default_rng(31 + N)
    th, x0 = _inputs(model, K, N, rng)
    obs, obs_bin = _masked(model, H, pattern, rng)
    row0 = 2 ** 32 - 3 * N          # the rows cross 2^32
    full = _run(model, th, x0, obs, obs_bin, N, row0=row0)
    _same(full, _run(model, th, x0, obs, obs_bin, N, row0=row0))
    assert np.isfinite(full["loglik"]).all() and (full["q"] > 0).any()
    boot = _run(model, th, x0, obs, obs_bin, N, row0=row0, proposal="bootstrap")
    assert not np.array_equal(boot["loglik"], full["loglik"])          # another filter, not an alias
    a = _run(model, th, x0, obs[:, :50], obs_bin[:, :50], N, row0=row0)
    b = _run(model, th, a["state_end"], obs, obs_bin, N, row0=row0, t0=50, loglik_in=a["loglik"])
    assert b["cloud"].shape[2] == 81
    for k, axis in (("ll_inc", 1), ("ess", 1), ("cloud", 2), ("q", 1), ("anc", 1)):
        assert np.array_equal(_bits(np.concatenate([a[k], b[k]], axis)), _bits(full[k])), k
    _same(b, full, keys=("loglik", "state_end"))
    _same(_run(model, th, x0, obs, obs_bin, N, row0=row0, cloud=False, trace=False), full,
          keys=("loglik", "ll_inc", "ess", "state_end"))
    sub = _run(model, th[2:], x0[2 * N:], obs, obs_bin, N, row0=row0 + 2 * N)       # filters 2 .. 4 alone
    for k in ("loglik", "ll_inc", "ess", "q", "anc"):
        assert np.array_equal(_bits(sub[k]), _bits(full[k][2:])), k
    for k in ("state_end", "cloud"):
        assert np.array_equal(_bits(sub[k]), _bits(full[k][2 * N:])), k
    one = _run(model, th[3:4], x0[3 * N:4 * N], obs, obs_bin, N, row0=row0 + 3 * N)  # one filter alone
    assert np.array_equal(_bits(one["loglik"]), _bits(full["loglik"][3:4]))
    assert np.array_equal(_bits(one["cloud"]), _bits(full["cloud"][3 * N:4 * N]))
    other = _run(model, th, x0, obs, obs_bin, N, row0=row0 + 1)
    assert not np.array_equal(other["cloud"], full["cloud"])


# ----------------------------------------------------------------------------------------------------------------
# 4. degenerate and dead
# ----------------------------------------------------------------------------------------------------------------
def test_observation_forty_sd_away_stays_finite():
    """AR: an observation forty predictive sd (sqrt(Sigma + R)) above every particle's predictive mean.  Every logw
    is below -800, the maximum still quantises to 2^40, and the cloud follows the observation."""
    model, K, N, H = SU.AR, 3, 64, 4
    rng = np.random.default_rng(41)
    th, x0 = _inputs(model, K, N, rng)
    obs, obs_bin = _series(model, H, "none", rng)
    free = _run(model, th, x0, obs, obs_bin, N)
    f = np.exp(2.0 * th[:, 2].astype(np.float64)) + OBS_STD[model] ** 2
    mean1 = th[:, 1:2] * free["cloud"][:, 0, 0].reshape(K, N) + th[:, 0:1]
    obs[0, 1] = float(mean1.max() + 40.0 * math.sqrt(f.max()))
    obs_bin[0, 1] = 1.0
    r = _run(model, th, x0, obs, obs_bin, N)
    assert np.array_equal(_bits(r["cloud"][:, :, 0]), _bits(free["cloud"][:, :, 0]))
    assert np.isfinite(r["loglik"]).all() and np.isfinite(r["cloud"]).all() and np.isfinite(r["ess"]).all()
    assert np.all(r["q"][:, 1].max(1) == ONE) and np.all(r["ll_inc"][:, 1] <= -0.5 * 40.0 ** 2)
    assert np.all(np.abs(r["loglik"] - r["ll_inc"][:, 1]) <= 2.0 ** -20 * np.abs(r["loglik"]))
    for k in range(K):
        want, _ = PR.systematic_ints(r["q"][k, 1], _resample_u(SEED, 1, k * N))
        assert r["anc"][k, 1].tolist() == want
    # the conditional mean closes Sigma / (Sigma + R) >= 0.8 of each particle's gap: all end beyond half of it
    assert np.all(r["cloud"][:, 0, 1] > mean1.max() + 20.0 * math.sqrt(f.max()))


def test_dying_particles_get_no_weight():
    """LV started next to the boundary (tests/test_gpu_particle.py's case): particles leave the positive orthant
    between observations, and a conditional draw may leave it after the resampling, so the adapted cloud holds NaN
    particles at observed steps too.  A particle whose pre-step state is NaN has q = 0 and is never an ancestor; the
    ancestors' pre-step states are alive; n_valid of the column summary is the count of finite rows."""
    from viforssms_amd.summary import column_summary
    model, K, N, H = SU.LV, 3, 128, 40
    rng = np.random.default_rng(12)
    th = np.tile(np.asarray(SU.TRUE_THETA[model], np.float32), (K, 1))
    x0 = np.stack([rng.uniform(0.1, 1.5, K * N), np.full(K * N, 100.0)], 1).astype(np.float32)
    obs = -np.ones((2, H), np.float32)
    obs_bin = np.zeros((2, H), np.float32)
    free = _run(model, th, x0, obs, obs_bin, N)
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
        assert np.all(r["ess"][:, t] >= 1.0) and np.all(r["ess"][:, t] <= N - before.sum(1))
        # (a slot dead after the step is a draw that left the orthant: its ancestor, with q > 0, was alive)
    assert died > 0, "no particle died before an observation: nothing was checked"
    for t in range(1, H):
        if t not in steps:
            assert np.all(nan[:, 0, t] >= nan[:, 0, t - 1])               # between observations the dead stay dead
    s = column_summary(torch.as_tensor(cloud.reshape(K * N, 2 * H), device=DEV))
    assert np.array_equal(s["n_valid"], np.isfinite(cloud).sum(0).reshape(-1))
    assert s["n_valid"].min() < K * N


def test_dead_filter_finishes():
    """Filter 1 of 3 starts with every particle outside the domain: -inf, NaN throughout, its neighbours untouched;
    chained, it stays dead."""
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
    assert np.all(r["ll_inc"][1, :first] == 0.0) and np.all(r["ess"][1, :first] == N)
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


def test_refusals():
    from viforssms_amd import _lib, ops
    th, x0 = _inputs(SU.LV, 2, 64, np.random.default_rng(1))
    g = lambda a: torch.as_tensor(a, device=DEV)
    obs, b = g(np.zeros((2, 8), np.float32)), g(np.zeros((2, 8), np.float32))
    call = lambda **kw: ops.particle_filter(**{**dict(model_id=SU.LV, theta=g(th), x_start=g(x0), obs=obs, obs_bin=b,
                                                      dt=0.1, obs_std=1.0, N=64, seed=1, row0=0,
                                                      proposal="adapted"), **kw})
    r = call(H=0)
    assert tuple(r.cloud.shape) == (128, 2, 0) and torch.equal(r.state_end, g(x0)) and not r.loglik.any()
    with pytest.raises(_lib.VissmError, match="proposal"):
        call(proposal="optimal")
    with pytest.raises(_lib.VissmError, match="obs_std"):
        call(obs_std=0.0)
    with pytest.raises(_lib.VissmError, match="SV"):
        call(model_id=SU.SV, theta=g(np.zeros((2, 4), np.float32)))
    with pytest.raises(_lib.VissmError, match="particles"):
        call(N=96)
    with pytest.raises(_lib.VissmError, match="x_start"):
        call(x_start=g(x0[:64]))
    with pytest.raises(_lib.VissmError, match="horizon"):
        call(t0=5, H=4)


# ----------------------------------------------------------------------------------------------------------------
# 5. statistical
# ----------------------------------------------------------------------------------------------------------------
def test_log_evidence_agrees_with_the_adapted_reference_and_kalman():
    """AR fixture (T = 64, obs_std = 1), K = 256 filters of N = 256 at the generator's theta: pf_ref.stat_bars
    against the adapted reference's K_r = 1024 filters and the exact Kalman value, and the discriminating condition
    sd <= 0.25 * the bootstrap reference's sd (the references measure 0.114 against 0.94)."""
    K, N = 256, 256
    obs, obs_bin = PR.stat_case()
    th = np.tile(np.asarray(SU.TRUE_THETA[SU.AR], np.float32), (K, 1))
    x0 = np.asarray(SU.TRUE_X[SU.AR], np.float32)
    r = _run(SU.AR, th, x0, obs, obs_bin, N, row0=123456, trace=False, cloud=False, obs_std=1.0)
    ll = r["loglik"]
    assert np.isfinite(ll).all()
    ref, boot, L = GR.reference_logliks(1), PR.reference_logliks(101), PR.stat_kalman()
    mu, s, mu_r, s_r, s_b = ll.mean(), ll.std(ddof=1), ref.mean(), ref.std(ddof=1), boot.std(ddof=1)
    bars = PR.stat_bars(mu, s, K, mu_r, s_r, ref.size, L)
    print(f"L {L:.4f} mu {mu:.4f} s {s:.4f} mu_r {mu_r:.4f} s_r {s_r:.4f} s_boot {s_b:.4f} L - mu {L - mu:.4f} {bars}")
    assert all(bars.values()), bars
    assert s <= 0.25 * s_b, (s, s_b)
    assert np.all(np.abs(r["ll_inc"].astype(np.float64).sum(1) - ll) <= 64 * 2.0 ** -20 * np.abs(ll))
    assert np.all(r["ess"][:, obs_bin[0] == 0] == N) and np.all(r["ess"] >= 1.0) and np.all(r["ess"] <= N)


def test_log_evidence_agrees_with_the_reference_lv():
    """LV, both coordinates observed with obs_std = 2 every fifth step of T = 40 (gpf_ref.small_dataset), K = 256
    filters of N = 256: mean within 4 se of the adapted reference's, sd ratio in [0.8, 1.25]."""
    model, sd, mask, K, N = SU.LV, 2.0, (1, 1), 256, 256
    obs, obs_bin = GR.small_dataset(model, sd, mask)
    th = np.tile(np.asarray(SU.TRUE_THETA[model], np.float32), (K, 1))
    r = _run(model, th, np.asarray(SU.TRUE_X[model], np.float32), obs, obs_bin, N, row0=777, trace=False,
             cloud=False, obs_std=sd)
    ll, ref = r["loglik"], GR.small_logliks(model, sd, mask, "adapted")
    assert np.isfinite(ll).all()
    mu, s, mu_r, s_r = ll.mean(), ll.std(ddof=1), ref.mean(), ref.std(ddof=1)
    se = math.sqrt(s * s / K + s_r * s_r / ref.size)
    print(f"mu {mu:.4f} s {s:.4f} mu_r {mu_r:.4f} s_r {s_r:.4f} se {se:.4f}")
    assert abs(mu - mu_r) <= 4.0 * se and 0.8 <= s / s_r <= 1.25


def test_smoother_runs_on_the_adapted_cloud():
    """Bars (b) and (c) of tests/test_gpu_smooth.py on the adapted filter's cloud: at every step the mean of the
    trajectories within 0.2 smoothing sd of the RTS mean and the pooled sd within 0.85 .. 1.15 of the RTS sd."""
    from viforssms_amd import ops
    K, N, M = PS.STAT_K, PS.STAT_N, PS.STAT_M
    obs, obs_bin = PR.stat_case()
    g = lambda a: torch.as_tensor(a, device=DEV)
    th = g(np.tile(np.asarray(SU.TRUE_THETA[SU.AR], np.float32), (K, 1)))
    f = ops.particle_filter(SU.AR, th, g(np.asarray(SU.TRUE_X[SU.AR], np.float32)), g(obs), g(obs_bin), SU.DT[SU.AR],
                            1.0, N, SEED, 123456, proposal="adapted")
    r = ops.particle_smooth(SU.AR, th, f.cloud, SU.DT[SU.AR], M, SEED ^ 0xABCDEF, 123456)
    paths = r.paths.cpu().numpy().astype(np.float64).reshape(K, M, -1)
    assert np.isfinite(paths).all()
    rts = PS.stat_rts()
    mean, se, sd = PS.stat_moments(paths)
    bars = PS.stat_bars(mean, se, sd, mean, se, rts)
    print(f"(b) {bars['b'][1]:.4f} sd (c) {bars['c'][1][0]:.4f} .. {bars['c'][1][1]:.4f}")
    assert bars["b"][0] and bars["c"][0], bars


# ----------------------------------------------------------------------------------------------------------------
# 6. product
# ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["ar", "lv"])
def filtered(request):
    model = _model(request.param)
    return request.param, model, model.particle_filter(KF, NF, proposal="adapted")


def test_product_keys_shapes_and_by_hand_call(filtered):
    from viforssms_amd import ops
    from viforssms_amd.vi_ssm import FILTER_SEED_XOR
    family, model, got = filtered
    _, T, _, S = CASES[family]
    md = model.mdef
    assert sorted(got) == sorted(KEYS + ("filter/proposal",)) and str(got["filter/proposal"]) == "adapted"
    P = SU.P_OF[md.model_id]
    shapes = {"probs": (5,), "filter/loglik": (KF,), "filter/theta": (KF, P), "filter/ll_inc": (KF, T),
              "filter/ess": (KF, T), "filter/mean": (S, T), "filter/sd": (S, T), "filter/n_valid": (S, T),
              "filter/quantiles": (5, S, T)}
    for k, shp in shapes.items():
        assert got[k].shape == shp, k
    _, theta = model.sample_paths_theta(np.tile(0, model.p_local), step=model.global_step)
    th = theta.detach().float()[:KF].contiguous()
    assert np.array_equal(got["filter/theta"], th.cpu().numpy())
    obs, obs_bin, x0 = (torch.as_tensor(a, device=DEV) for a in model.filter_data)
    r = ops.particle_filter(md.model_id, th, x0, obs[:, :T].contiguous(), obs_bin[:, :T].contiguous(), md.dt,
                            md.obs_std, NF, model.engine.seed ^ FILTER_SEED_XOR, model.global_step * KF * NF,
                            proposal="adapted")
    assert np.array_equal(_bits(got["filter/loglik"]), _bits(r.loglik.cpu().numpy()))
    assert np.array_equal(_bits(got["filter/ll_inc"]), _bits(r.ll_inc.cpu().numpy()))
    assert np.isfinite(got["filter/loglik"]).any(), "every filter died: nothing is compared"
    assert np.array_equal(got["filter/n_valid"], np.isfinite(r.cloud.cpu().numpy()).sum(0))


def test_product_chunking_and_the_default(filtered):
    family, model, got = filtered
    for chunk in (7, 64):
        res = model.particle_filter(KF, NF, chunk=chunk, proposal="adapted")
        for k in got:
            assert _eq(res[k], got[k]), (chunk, k)
    # the default proposal: today's dict, bitwise the by-hand bootstrap launch, and no new key
    from viforssms_amd import _lib, ops
    from viforssms_amd.vi_ssm import FILTER_SEED_XOR
    base = model.particle_filter(KF, NF)
    assert sorted(base) == sorted(KEYS)
    named = model.particle_filter(KF, NF, proposal="bootstrap")
    for k in KEYS:
        assert _eq(base[k], named[k]), k
    md, T = model.mdef, CASES[family][1]
    obs, obs_bin, x0 = (torch.as_tensor(a, device=DEV) for a in model.filter_data)
    r = ops.particle_filter(md.model_id, torch.as_tensor(base["filter/theta"], device=DEV), x0,
                            obs[:, :T].contiguous(), obs_bin[:, :T].contiguous(), md.dt, md.obs_std, NF,
                            model.engine.seed ^ FILTER_SEED_XOR, model.global_step * KF * NF)
    assert np.array_equal(_bits(base["filter/loglik"]), _bits(r.loglik.cpu().numpy()))
    assert not np.array_equal(base["filter/loglik"], got["filter/loglik"])
    with pytest.raises(_lib.VissmError, match="proposal"):
        model.particle_filter(KF, NF, proposal="optimal")
    with pytest.raises(_lib.VissmError, match="proposal"):
        model.particle_smoother(KF, NF, 64, proposal="optimal")


def test_product_smoother_save_and_sv(filtered, tmp_path):
    from tests.parity_util import build_model
    family, model, got = filtered
    sm = model.particle_smoother(KF, NF, 64, proposal="adapted")
    for k in got:
        assert _eq(sm[k], got[k]), k
    assert sm["smooth/mean"].shape == got["filter/mean"].shape
    path = str(tmp_path / "sub" / "filter.npz")
    res = model.save_filter(path, KF, NF, proposal="adapted")
    with np.load(path) as z:
        assert sorted(z.files) == sorted(got) and str(z["filter/proposal"]) == "adapted"
        for k in got:
            assert _eq(z[k], got[k]) and _eq(res[k], got[k]), k
    if family == "ar":
        sv = build_model("sv", 7, 40, 8, 2, 16, 5, 3, DEV, T=160, precision=0, seed=3)
        with pytest.raises(ValueError, match="SV"):
            sv.particle_filter(4, 64, proposal="adapted")


def test_main_writes_the_adapted_filter(tmp_path, monkeypatch):
    """python main.py hyperparameters.txt ... --filter 4 64 PATH --filter-proposal adapted"""
    state = np.random.get_state()
    monkeypatch.chdir(tmp_path)
    try:
        import main
        out = str(tmp_path / "post" / "filter.npz")
        model = main.run([os.path.join(ROOT, "hyperparameters.txt"), "-T", "60", "-b", "30", "-k", "5", "-p", "8",
                          "-f", "4", "--steps", "2", "--no-pretrain", "--filter", "4", "64", out,
                          "--filter-proposal", "adapted"])
    finally:
        np.random.set_state(state)
    assert model.global_step == 2
    with np.load(out) as z:
        assert str(z["filter/proposal"]) == "adapted"
        assert z["filter/loglik"].shape == (4,) and z["filter/quantiles"].shape == (5, 1, 60)
        assert z["filter/ess"].shape == (4, 60) and np.all((z["filter/ess"] <= 64) | np.isnan(z["filter/ess"]))
