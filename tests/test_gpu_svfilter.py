"""vissm_sv_filter and vissm_sv_smooth (ops.sv_filter, ops.sv_smooth; PosteriorDiagnostics.volatility_filter /
volatility_smoother) on the GPU.

The filter is checked teacher-forced, step by step, against the float64 reference of tests/svf_ref.py applied to the
kernel's own previous cloud: the weights of the *pre-step* states within the q bar of tests/test_gpu_particle.py, the
ancestors exactly (Python-int systematic resampling of the traced weights), the moved states within tests/sim_util.py's
state bar of the float64 move of the ancestor's state with the slot's own normal.  Repeated, chunked and sub-batched
launches are compared bitwise; a dead filter ends -inf / NaN next to untouched neighbours; the log-evidence estimates
meet the three statistical bars against the reference's and the grid value.  The smoother's every selected index is
reproduced from the traced weights, chunked equals whole, a dead filter gives NaN trajectories and the bands meet the
grid smoother within the bars tests/test_gpu_smooth.py holds against RTS.  Then the product path."""
import math
import os

import numpy as np
import pytest
import torch

from tests import pf_ref as PR
from tests import ps_ref as PS
from tests import svf_ref as R
from tests.sim_util import (PF_ONE as ONE, PF_SEED as SEED, bits as _bits, resample_u as _resample_u,
                            same_bits as _same, state_bar as _bar)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 1.0


def _inputs(K, N, H, rng):
    """theta [K, 4] within 0.1 of PARAM_INIT, start states [K N] within 1 of h_0 = -8.5, and a series y[0 .. H]
    simulated from the model at PARAM_INIT."""
    th = (np.asarray(R.PARAM_INIT) + rng.uniform(-0.1, 0.1, (K, 4))).astype(np.float32)
    h0 = (R.FIX_H0 + rng.uniform(-1.0, 1.0, K * N)).astype(np.float32)
    y, _ = R.simulate_series(H, R.PARAM_INIT, DT, R.FIX_H0, 1.0, rng)
    return th, h0, y


def _run(th, h0, y, N, row0=0, t0=0, H=None, loglik_in=None, cloud=True, trace=True, seed=SEED):
    from viforssms_amd import ops
    g = lambda a: torch.as_tensor(np.array(a), device=DEV)
    r = ops.sv_filter(g(th), g(h0), g(y), DT, N, seed, row0, t0=t0,
                      loglik_in=None if loglik_in is None else g(loglik_in), cloud=cloud, H=H, trace=trace)
    torch.cuda.synchronize()
    c = lambda t: None if t is None else t.cpu().numpy()
    return {"loglik": c(r.loglik), "ll_inc": c(r.ll_inc), "ess": c(r.ess), "state_end": c(r.state_end),
            "cloud": c(r.cloud), "q": c(r.q_trace), "anc": c(r.anc_trace)}


def _smooth(th, cloud, y, M, row0=0, t0=0, x_next=None, idx=True, trace=False, seed=SEED):
    from viforssms_amd import ops
    g = lambda a: None if a is None else torch.as_tensor(np.array(a), device=DEV)
    r = ops.sv_smooth(g(th), g(cloud), g(y), DT, M, seed, row0, t0=t0, x_next=g(x_next), idx=idx, trace=trace)
    torch.cuda.synchronize()
    c = lambda t: None if t is None else t.cpu().numpy()
    return {"paths": c(r.paths), "x_first": c(r.x_first), "idx": c(r.idx), "q": c(r.q_trace)}


def _select_u(seed, t_abs, rows):
    """The smoother's selection words of Philox rows `rows` at absolute step t_abs (counter word 2)."""
    from tests import philox_ref
    rows = np.asarray(rows, np.uint64)
    ctr = np.zeros(rows.shape + (4,), np.uint64)
    ctr[..., 0], ctr[..., 1] = t_abs, 2
    ctr[..., 2], ctr[..., 3] = rows & philox_ref.M32, rows >> philox_ref.SH32
    return philox_ref.philox4x32_10(ctr, np.asarray([seed & 0xFFFFFFFF, seed >> 32], np.uint64))[..., 0]


def _q_tol(qref, lw64, lw32, m64, live):
    """tests/test_gpu_particle.py's q bar: logw and m each within d = 8 max(e32, 2^-20 mean |logw|), the fp32 exp and
    the truncation on top."""
    d = 8.0 * max(float(np.max(np.abs(lw32 - lw64)[live])), 2.0 ** -20 * float(np.mean(np.abs(lw64[live]))))
    with np.errstate(invalid="ignore"):
        gap = np.where(live, np.abs(lw64 - m64), 0.0)
    return qref.astype(np.float64) * (math.expm1(2.0 * d) + (gap + 2.0) * 2.0 ** -23) + 1.0


# ----------------------------------------------------------------------------------------------------------------
# 1. teacher-forced parity
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,H", [(3, 64, 65), (1, 1024, 131), (3, 128, 1), (1, 128, 63), (3, 1024, 64),
                                     (3, 256, 65), (1, 512, 65)])
def test_teacher_forced_parity(K, N, H):
    from viforssms_amd import ops
    rng = np.random.default_rng(10 * N + H + K)
    th, h0, y = _inputs(K, N, H, rng)
    row0 = 3 + 7 * N
    r = _run(th, h0, y, N, row0=row0)
    eps, _ = ops.normal_base(SEED, row0, K * N, H, 0, DEV)
    nn = eps.cpu().numpy().reshape(K * N, H)
    th_rows = np.repeat(th, N, 0)
    th64 = th_rows.astype(np.float64)
    cloud, anc, q = r["cloud"], r["anc"].astype(np.int64), r["q"]
    assert cloud.shape == (K * N, 1, H) and np.isfinite(cloud).all()
    exp64, exp32 = np.empty((K * N, 1, H)), np.empty((K * N, 1, H), np.float32)
    prev = h0
    shares = {"q": 0.0, "ll_inc": 0.0, "ess": 0.0}
    ll_sum, ll_bar = np.zeros(K), np.zeros(K)
    for t in range(H):
        lw32_all = R.state_logw(prev, y[t], y[t + 1], th_rows, DT, np.float32).astype(np.float64)
        for k in range(K):
            sl = slice(k * N, (k + 1) * N)
            alive, lw64, m64, qref = R.weigh(prev[sl].astype(np.float64), y[t], y[t + 1], th64[sl], DT)
            assert alive.all()
            qk = [int(v) for v in q[k, t]]
            want_anc, W = PR.systematic_ints(qk, _resample_u(SEED, t, row0 + k * N))
            assert W > 0 and max(qk) == ONE
            assert anc[k, t].tolist() == want_anc, (k, t)
            tol = _q_tol(qref, lw64, lw32_all[sl], m64, alive)
            err = np.abs(np.asarray(qk, np.float64) - qref.astype(np.float64))
            assert np.all(err <= tol), (k, t, float(np.max(err / tol)))
            shares["q"] = max(shares["q"], float(np.max(err / tol)))
            v = PR.ll_increment(m64, W, N)
            bar = 8.0 * max(float(np.max(np.abs(lw32_all[sl] - lw64))), 2.0 ** -20 * abs(v))
            assert abs(float(r["ll_inc"][k, t]) - v) <= bar, (k, t)
            shares["ll_inc"] = max(shares["ll_inc"], abs(float(r["ll_inc"][k, t]) - v) / bar)
            ll_sum[k] += v
            ll_bar[k] += bar
            e = PR.ess(qk)
            assert abs(float(r["ess"][k, t]) - e) <= 8.0 * 2.0 ** -20 * e and 1.0 <= e <= N, (k, t)
            shares["ess"] = max(shares["ess"], abs(float(r["ess"][k, t]) - e) / (8.0 * 2.0 ** -20 * e))
        rows = (np.arange(K)[:, None] * N + anc[:, t, :]).reshape(-1)
        ha = prev[rows]
        exp64[:, 0, t] = R.h_step(ha.astype(np.float64), th64, DT, nn[:, t].astype(np.float64))
        exp32[:, 0, t] = R.h_step(ha, th_rows, DT, nn[:, t], np.float32)
        prev = cloud[:, 0, t]
    bar, e32 = _bar(exp64, exp32)
    dev = np.abs(cloud - exp64)
    print(f"K {K} N {N} H {H}: e32 {e32:.3e}, shares of the bars: cloud {np.max(dev / bar):.3f} q {shares['q']:.3f} "
          f"ll_inc {shares['ll_inc']:.3f} ess {shares['ess']:.3f}")
    assert np.all(dev <= bar)
    assert np.all(np.abs(r["loglik"] - ll_sum) <= ll_bar + 1e-12)
    assert np.array_equal(_bits(r["state_end"]), _bits(cloud[:, :, -1]))


# ----------------------------------------------------------------------------------------------------------------
# 2. bitwise
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [64, 128, 1024])
def test_bitwise_repeat_chunks_and_sub_batch(N):
    K, H = 3, 131
    rng = np.random.default_rng(31 + N)
    th, h0, y = _inputs(K, N, H, rng)
    row0 = 2 ** 32 - 2 * N          # the rows cross 2^32
    full = _run(th, h0, y, N, row0=row0)
    _same(full, _run(th, h0, y, N, row0=row0))
    assert np.isfinite(full["loglik"]).all() and (full["q"] > 0).any()
    a = _run(th, h0, y, N, row0=row0, H=64)
    b = _run(th, a["state_end"], y, N, row0=row0, t0=64, loglik_in=a["loglik"])
    assert b["cloud"].shape[2] == 67
    for k, axis in (("ll_inc", 1), ("ess", 1), ("cloud", 2), ("q", 1), ("anc", 1)):
        assert np.array_equal(_bits(np.concatenate([a[k], b[k]], axis)), _bits(full[k])), k
    _same(b, full, keys=("loglik", "state_end"))
    _same(_run(th, h0, y, N, row0=row0, cloud=False, trace=False), full, keys=("loglik", "ll_inc", "ess", "state_end"))
    for k in range(K):                                                   # each filter alone, on its row
        one = _run(th[k:k + 1], h0[k * N:(k + 1) * N], y, N, row0=row0 + k * N)
        for key in ("loglik", "ll_inc", "ess", "q", "anc"):
            assert np.array_equal(_bits(one[key]), _bits(full[key][k:k + 1])), (k, key)
        assert np.array_equal(_bits(one["cloud"]), _bits(full["cloud"][k * N:(k + 1) * N])), k
    other = _run(th, h0, y, N, row0=row0 + 1)
    assert not np.array_equal(other["cloud"], full["cloud"])
    # a longer series changes nothing: steps past t0 + H are not read
    longer = np.concatenate([y, np.full(5, np.nan, np.float32)])
    _same(_run(th, h0, longer, N, row0=row0, H=H), full)


def test_dead_filter_and_degenerate_series():
    """Filter 1 of 3 starts with every particle NaN or infinite: -inf, NaN throughout, its neighbours untouched;
    chained, it stays dead.  A zero in the series kills every filter at that step (the product refuses it first)."""
    K, N, H = 3, 128, 70
    rng = np.random.default_rng(43)
    th, h0, y = _inputs(K, N, H, rng)
    good = _run(th, h0, y, N)
    bad0 = h0.copy()
    bad0[N:2 * N] = np.where(np.arange(N) % 2 == 0, np.inf, np.nan)
    r = _run(th, bad0, y, N)
    assert r["loglik"][1] == -np.inf and np.isfinite(r["loglik"][[0, 2]]).all()
    assert np.isnan(r["cloud"][N:2 * N]).all() and np.isnan(r["state_end"][N:2 * N]).all()
    assert np.isnan(r["ll_inc"][1]).all() and np.isnan(r["ess"][1]).all() and not r["q"][1].any()
    for k in (0, 2):
        for key in ("ll_inc", "ess", "q", "anc"):
            assert np.array_equal(_bits(r[key][k]), _bits(good[key][k])), (k, key)
        assert np.array_equal(_bits(r["cloud"][k * N:(k + 1) * N]), _bits(good["cloud"][k * N:(k + 1) * N]))
    a = _run(th, bad0, y, N, H=30)
    b = _run(th, a["state_end"], y, N, t0=30, loglik_in=a["loglik"])
    assert b["loglik"][1] == -np.inf and np.isnan(b["ll_inc"][1]).all()
    _same(b, r, keys=("loglik", "state_end"))
    assert np.array_equal(_bits(np.concatenate([a["cloud"], b["cloud"]], 2)), _bits(r["cloud"]))
    # some particles dead at the start: no weight, never an ancestor
    part = h0.copy().reshape(K, N)
    part[:, ::3] = np.nan
    p = _run(th, part.reshape(-1), y, N)
    assert np.isfinite(p["loglik"]).all() and np.isfinite(p["cloud"]).all()
    assert not p["q"][:, 0, ::3].any() and np.all(p["anc"][:, 0] % 3 != 0)
    y0 = y.copy()
    y0[20] = 0.0
    z = _run(th, h0, y0, N)
    assert np.all(z["loglik"] == -np.inf) and np.isnan(z["cloud"][:, :, 20:]).all()
    # (step 19 reads y[20] as its new observation and stays finite; step 20 has it as y_prev)
    assert np.isfinite(z["cloud"][:, :, :20]).all()
    assert np.array_equal(_bits(z["cloud"][:, :, :19]), _bits(good["cloud"][:, :, :19]))


def test_refusals():
    from viforssms_amd import _lib, ops
    th, h0, y = _inputs(2, 64, 8, np.random.default_rng(1))
    g = lambda a: torch.as_tensor(a, device=DEV)
    call = lambda **kw: ops.sv_filter(**{**dict(theta=g(th), x_start=g(h0), obs=g(y), dt=1.0, N=64, seed=1, row0=0),
                                         **kw})
    r = call(H=0)
    assert tuple(r.cloud.shape) == (128, 1, 0) and torch.equal(r.state_end[:, 0], g(h0)) and not r.loglik.any()
    one = call(x_start=g(np.float32([-8.5])))
    assert tuple(one.cloud.shape) == (128, 1, 8) and torch.isfinite(one.loglik).all()
    with pytest.raises(_lib.VissmError, match="particles"):
        call(N=96)
    with pytest.raises(_lib.VissmError, match="x_start"):
        call(x_start=g(h0[:64]))
    with pytest.raises(_lib.VissmError, match="horizon"):
        call(t0=5, H=4)
    with pytest.raises(_lib.VissmError, match="theta"):
        call(theta=g(th[:, :3].copy()))
    with pytest.raises(_lib.VissmError, match="dt"):
        call(dt=0.0)
    with pytest.raises(_lib.VissmError, match="horizon"):
        ops.sv_smooth(g(th), one.cloud, g(y), 1.0, 64, 1, 0, t0=1)                 # y[10] of y[0 .. 8]
    with pytest.raises(_lib.VissmError, match="horizon"):
        ops.sv_smooth(g(th), one.cloud, g(y), 1.0, 64, 1, 0, x_next=one.state_end[:128].contiguous())
    with pytest.raises(_lib.VissmError, match="trajectories"):
        ops.sv_smooth(g(th), one.cloud, g(y), 1.0, 128, 1, 0)


# ----------------------------------------------------------------------------------------------------------------
# 3. statistical
# ----------------------------------------------------------------------------------------------------------------
def test_log_evidence_agrees_with_the_reference_and_the_grid():
    """The fixture (T = 64 at PARAM_INIT), K = 256 filters of N = 256: pf_ref.stat_bars against the reference's
    K_r = 1024 estimates stored in the fixture and the grid value."""
    K, N = 256, R.FIX_N
    z = R.fixture()
    L, _, _ = R.fixture_truth()
    th = np.tile(np.asarray(R.PARAM_INIT, np.float32), (K, 1))
    r = _run(th, np.float32([R.FIX_H0]), z["y"], N, row0=123456, trace=False, cloud=False)
    ll, ref = r["loglik"], z["ref_logliks"]
    assert np.isfinite(ll).all()
    mu, s, mu_r, s_r = ll.mean(), ll.std(ddof=1), ref.mean(), ref.std(ddof=1)
    bars = PR.stat_bars(mu, s, K, mu_r, s_r, ref.size, L)
    print(f"L {L:.4f} mu {mu:.4f} s {s:.4f} mu_r {mu_r:.4f} s_r {s_r:.4f} L - mu {L - mu:.4f} {bars}")
    assert all(bars.values()), bars
    assert np.all(np.abs(r["ll_inc"].astype(np.float64).sum(1) - ll) <= 64 * 2.0 ** -20 * np.abs(ll))
    assert np.all(r["ess"] >= 1.0) and np.all(r["ess"] <= N)


# ----------------------------------------------------------------------------------------------------------------
# 4. smoother
# ----------------------------------------------------------------------------------------------------------------
def _check_smooth(th, cloud, y, r, K, N, M, row0=0, t0=0, x_next=None, seed=SEED, q_steps=()):
    """The gather identity everywhere; with a trace the exact selection everywhere and the q bar at q_steps."""
    H = cloud.shape[2]
    cl, paths, idx = cloud.reshape(K, N, H), r["paths"].reshape(K, M, H), r["idx"].reshape(K, M, H)
    assert np.array_equal(_bits(r["x_first"][:, 0]), _bits(r["paths"][:, 0, 0]))
    share = 0.0
    for k in range(K):
        for t in range(H - 1, -1, -1):
            h, ix = cl[k, :, t], idx[k, :, t].astype(np.int64)
            alive, drawn = np.isfinite(h), ix >= 0
            assert np.all(ix[drawn] < N) and alive[ix[drawn]].all(), (k, t)
            assert np.array_equal(_bits(paths[k, drawn, t]), _bits(h[ix[drawn]])), (k, t)
            assert np.isnan(paths[k, ~drawn, t]).all(), (k, t)
            if r["q"] is None:
                continue
            terminal = t == H - 1 and x_next is None
            target = None if terminal else (paths[k, :, t + 1] if t < H - 1 else x_next.reshape(K, M)[k])
            U = _select_u(seed, t0 + t, row0 + k * N + np.arange(M))
            qk = r["q"][k, t].astype(np.uint64)
            want, W = PS.select_u64(qk, U)
            assert np.array_equal(ix, want), (k, t)
            for j in (0, M // 2 + 1, M - 1):
                assert PS.select_ints(qk[j], int(U[j]))[0] == ix[j], (k, t, j)
            assert not qk[:, ~alive].any() and np.all(qk.max(1)[W > 0] == ONE), (k, t)
            if t not in q_steps:
                continue
            ca = t0 + t
            y1, y2 = (0.0, 0.0) if terminal else (y[ca + 1], y[ca + 2])
            _, lw64, m64, qref, _ = R.backward_draw(h.astype(np.float64), None if terminal else
                                                    target.astype(np.float64), th[k].astype(np.float64), DT, y1, y2, U,
                                                    terminal)
            if terminal:
                lw32 = np.zeros_like(lw64)
            else:
                lw32 = R.backward_logw(h[None, :], target[:, None], th[k], DT, y1, y2, np.float32).astype(np.float64)
            live = np.broadcast_to(alive[None, :], lw64.shape) & np.isfinite(lw64)
            assert live.any()
            tol = _q_tol(qref, lw64, lw32, m64[:, None], live)
            err = np.abs(qk.astype(np.float64) - qref.astype(np.float64))
            assert np.all(err <= tol), (k, t, float(np.max(err / tol)))
            share = max(share, float(np.max(err / tol)))
    return share


@pytest.mark.parametrize("N,M,H,K", [(64, 64, 131, 3), (128, 64, 64, 1), (1024, 1024, 9, 1), (256, 128, 33, 2),
                                     (512, 64, 17, 1), (128, 128, 1, 3)])
def test_smoother_selection_is_reproduced(N, M, H, K):
    """Over the filter's own cloud, with a fifth of the particles of filter 0 knocked out (NaN) at two columns."""
    rng = np.random.default_rng(7 * N + M + H)
    th, h0, y = _inputs(K, N, H + 1, rng)            # one more observation than columns: y[ca + 2] exists everywhere
    cloud = _run(th, h0, y, N, row0=11, H=H, trace=False)["cloud"].copy()
    for t in {0, H // 2}:
        cloud[rng.choice(N, N // 5, replace=False), 0, t] = np.nan
    r = _smooth(th, cloud, y, M, row0=11, trace=True)
    share = _check_smooth(th, cloud, y, r, K, N, M, row0=11, q_steps={0, H // 2, H - 2, H - 1} & set(range(H)))
    assert np.isfinite(r["paths"]).all()
    print(f"N {N} M {M} H {H} K {K}: largest share of the q bar {share:.3f}")
    # with a target after the last column
    xn = (R.FIX_H0 + rng.uniform(-1.0, 1.0, (K * M, 1))).astype(np.float32)
    r2 = _smooth(th, cloud, y, M, row0=11, x_next=xn, trace=True)
    _check_smooth(th, cloud, y, r2, K, N, M, row0=11, x_next=xn, q_steps={H - 1})


@pytest.mark.parametrize("N,M", [(64, 64), (1024, 128)])
def test_smoother_bitwise_chunks_and_dead_filter(N, M):
    K, H = 3, 131
    rng = np.random.default_rng(5 + N)
    th, h0, y = _inputs(K, N, H, rng)
    row0 = 2 ** 32 - N
    f = _run(th, h0, y, N, row0=row0, trace=False)
    cloud = f["cloud"]
    whole = _smooth(th, cloud, y, M, row0=row0)
    _same(whole, _smooth(th, cloud, y, M, row0=row0), keys=("paths", "x_first", "idx"))
    b = _smooth(th, np.ascontiguousarray(cloud[:, :, 64:]), y, M, row0=row0, t0=64)
    a = _smooth(th, np.ascontiguousarray(cloud[:, :, :64]), y, M, row0=row0, t0=0, x_next=b["x_first"])
    assert np.array_equal(_bits(np.concatenate([a["paths"], b["paths"]], 2)), _bits(whole["paths"]))
    assert np.array_equal(_bits(np.concatenate([a["idx"], b["idx"]], 1)), _bits(whole["idx"]))
    assert np.array_equal(_bits(a["x_first"]), _bits(whole["x_first"]))
    one = _smooth(th[1:2], cloud[N:2 * N], y, M, row0=row0 + N)          # filter 1 alone, on its row
    assert np.array_equal(_bits(one["paths"]), _bits(whole["paths"][M:2 * M]))
    # a filter that died half way: NaN from there on, hence NaN trajectories throughout; its neighbours untouched
    dead = cloud.copy()
    dead[N:2 * N, :, 70:] = np.nan
    d = _smooth(th, dead, y, M, row0=row0)
    assert np.isnan(d["paths"][M:2 * M]).all() and np.all(d["idx"][M:2 * M] == -1)
    for k in (0, 2):
        assert np.array_equal(_bits(d["paths"][k * M:(k + 1) * M]), _bits(whole["paths"][k * M:(k + 1) * M]))


def test_smoothing_bands_match_the_grid_smoother():
    """The fixture, K = 256 filters of N = 256, M = 64 trajectories each: bars (b) and (c) of tests/ps_ref.py against
    the grid smoother -- the mean within 0.2 smoothing sd and the pooled sd within 0.85 .. 1.15 at every step."""
    K, N, M = PS.STAT_K, PS.STAT_N, PS.STAT_M
    z = R.fixture()
    _, ms, sds = R.fixture_truth()
    th = np.tile(np.asarray(R.PARAM_INIT, np.float32), (K, 1))
    f = _run(th, np.float32([R.FIX_H0]), z["y"], N, row0=123456, trace=False)
    r = _smooth(th, f["cloud"], z["y"], M, row0=123456, seed=SEED ^ 0xABCDEF, idx=False)
    paths = r["paths"].astype(np.float64).reshape(K, M, -1)
    assert np.isfinite(paths).all()
    mean, _, sd = PS.stat_moments(paths)
    bars = R.smooth_bars(mean, sd, ms, sds)
    print(f"(b) {bars['b'][1]:.4f} sd (c) {bars['c'][1][0]:.4f} .. {bars['c'][1][1]:.4f}")
    assert bars["b"][0] and bars["c"][0], bars
    # the filtering bands sit on the grid's filtering moments in the same way
    cl = f["cloud"].astype(np.float64).reshape(K, N, -1)
    fm, _, fsd = PS.stat_moments(cl)
    fb = R.smooth_bars(fm, fsd, z["grid_mf"][1], z["grid_sdf"][1])
    assert fb["b"][0] and fb["c"][0], fb


# ----------------------------------------------------------------------------------------------------------------
# 5. product
# ----------------------------------------------------------------------------------------------------------------
KF, NF, MF, T = 4, 64, 64, 160
FKEYS = ("probs", "filter/loglik", "filter/theta", "filter/ll_inc", "filter/ess", "filter/mean", "filter/sd",
         "filter/n_valid", "filter/quantiles", "filter/proposal")
SKEYS = ("smooth/mean", "smooth/sd", "smooth/n_valid", "smooth/quantiles")


def _eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


@pytest.fixture(scope="module")
def sv_model():
    from tests.parity_util import build_model
    return build_model("sv", 7, 40, 8, 2, 16, 5, 3, DEV, T=T, precision=0, seed=3)


def test_product_filter_and_smoother(sv_model, tmp_path):
    from viforssms_amd import ops
    from viforssms_amd.diagnostics import FILTER_SEED_XOR
    model = sv_model
    got = model.volatility_filter(KF, NF)
    assert sorted(got) == sorted(FKEYS) and str(got["filter/proposal"]) == "adapted"
    shapes = {"probs": (5,), "filter/loglik": (KF,), "filter/theta": (KF, 4), "filter/ll_inc": (KF, T),
              "filter/ess": (KF, T), "filter/mean": (1, T), "filter/sd": (1, T), "filter/n_valid": (1, T),
              "filter/quantiles": (5, 1, T)}
    for k, shp in shapes.items():
        assert got[k].shape == shp, k
    _, theta = model.sample_paths_theta(np.tile(0, model.p_local), step=model.global_step)
    th = theta.detach().float()[:KF].contiguous()
    assert np.array_equal(got["filter/theta"], th.cpu().numpy())
    y = torch.as_tensor(np.asarray(model.obs, np.float32)[:T + 1], device=DEV)
    r = ops.sv_filter(th, torch.full((1,), model.x0, device=DEV), y, model.mdef.dt, NF,
                      model.engine.seed ^ FILTER_SEED_XOR, model.global_step * KF * NF)
    assert np.array_equal(_bits(got["filter/loglik"]), _bits(r.loglik.cpu().numpy()))
    assert np.array_equal(_bits(got["filter/ll_inc"]), _bits(r.ll_inc.cpu().numpy()))
    assert np.array_equal(got["filter/n_valid"], np.isfinite(r.cloud.cpu().numpy()).sum(0))
    assert np.isfinite(got["filter/loglik"]).any(), "every filter died: nothing is compared"
    sm = model.volatility_smoother(KF, NF, MF)
    assert sorted(sm) == sorted(FKEYS + SKEYS)
    for k in FKEYS:                                  # the forward pass is the filter's, bitwise
        assert _eq(sm[k], got[k]), k
    assert sm["smooth/mean"].shape == (1, T) and sm["smooth/quantiles"].shape == (5, 1, T)
    assert sm["smooth/n_valid"].max() == KF * MF or not np.isfinite(got["filter/loglik"]).all()
    summary = model.posterior_summary()
    # lays directly over the fit's bands of the latent coordinate (the summary's first is the observed series)
    assert summary["paths/quantiles"][:, 1:].shape == sm["smooth/quantiles"].shape
    for chunk in (7, 64):
        res = model.volatility_filter(KF, NF, chunk=chunk)
        for k in got:
            assert _eq(res[k], got[k]), (chunk, k)
        res = model.volatility_smoother(KF, NF, MF, chunk=chunk)
        for k in sm:
            assert _eq(res[k], sm[k]), (chunk, k)
    for name, want, save in (("filter.npz", got, lambda p: model.save_volatility_filter(p, KF, NF)),
                             ("smooth.npz", sm, lambda p: model.save_volatility_smoother(p, KF, NF, MF))):
        path = str(tmp_path / "sub" / name)
        res = save(path)
        with np.load(path) as z:
            assert sorted(z.files) == sorted(want)
            for k in want:
                assert _eq(z[k], want[k]) and _eq(res[k], want[k]), k
    # the existing entries still refuse SV
    with pytest.raises(ValueError, match="SV"):
        model.particle_filter(KF, NF)
    with pytest.raises(ValueError, match="SV"):
        model.particle_smoother(KF, NF, MF)


def test_product_refusals(sv_model):
    from tests.parity_util import FILTER_KF, FILTER_NF, filter_model
    model = sv_model
    with pytest.raises(ValueError, match="n_particles"):
        model.volatility_filter(KF, 96)
    with pytest.raises(ValueError, match="n_theta"):
        model.volatility_filter(model.p_local + 1, NF)
    with pytest.raises(ValueError, match="n_paths"):
        model.volatility_smoother(KF, NF, 128)
    keep = model.obs
    try:
        for t, v, what in ((17, 0.0, "= 0"), (T - 1, 0.0, "= 0"), (5, np.nan, "finite"), (T, np.inf, "finite")):
            model.obs = keep.copy()
            model.obs[t] = v
            with pytest.raises(ValueError, match=what):
                model.volatility_filter(KF, NF)
            with pytest.raises(ValueError, match=what):
                model.volatility_smoother(KF, NF, MF)
        model.obs = keep.copy()
        model.obs[T] = 0.0                                  # the last value is never a y_prev: allowed
        assert model.volatility_filter(KF, NF)["filter/ll_inc"].shape == (KF, T)
    finally:
        model.obs = keep
    ar = filter_model("ar")
    with pytest.raises(ValueError, match="particle_filter"):
        ar.volatility_filter(FILTER_KF, FILTER_NF)
    with pytest.raises(ValueError, match="particle_filter"):
        ar.volatility_smoother(FILTER_KF, FILTER_NF, 64)


def test_run_writes_the_filter_and_the_smoother(tmp_path, monkeypatch):
    """viforssms_amd.sv.run (SV_dense.py's driver) ... --filter 4 64 PATH --smooth 4 64 64 PATH"""
    from viforssms_amd import sv
    state = np.random.get_state()
    monkeypatch.chdir(tmp_path)
    try:
        out, out2 = str(tmp_path / "post" / "filter.npz"), str(tmp_path / "post" / "smooth.npz")
        model = sv.run(["-p", "8", "--kernel-len", "8", "--batch-dims", "26", "--no-flows", "2", "--feat-window", "3",
                        "--steps", "2", "--no-pretrain", "--filter", "4", "64", out, "--smooth", "4", "64", "64", out2])
    finally:
        np.random.set_state(state)
    assert model.global_step == 2
    n = model.target_len()
    with np.load(out) as z, np.load(out2) as z2:
        assert str(z["filter/proposal"]) == "adapted"
        assert z["filter/loglik"].shape == (4,) and z["filter/quantiles"].shape == (5, 1, n)
        assert z["filter/ess"].shape == (4, n) and np.all((z["filter/ess"] <= 64) | np.isnan(z["filter/ess"]))
        assert z2["smooth/quantiles"].shape == (5, 1, n) and _eq(z2["filter/loglik"], z["filter/loglik"])
