"""The stochastic-volatility particle filter and smoother without a GPU: csrc/svf_math.hpp (the code the kernels run,
built for the host in libvissm_hostcheck.so) against the float64 formulas of tests/svf_ref.py; the move against
sim::em_step<SV> bit for bit; one serial filter step and one serial backward draw against Python-int arithmetic; every
refusal of vissm_sv_filter, vissm_sv_smooth and their *_lds_bytes functions, which are host arithmetic; and the
statistical bars of tests/test_gpu_svfilter.py for the numpy reference alone, against the grid forward-backward pass."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import pf_ref as PR
from tests import ps_ref as PS
from tests import sim_util as SU
from tests import svf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK = os.path.join(ROOT, "viforssms_amd", "libvissm_hostcheck.so")
FP = ctypes.POINTER(ctypes.c_float)
NPTS = 256


@pytest.fixture(scope="module")
def hc():
    lib = ctypes.CDLL(HOSTCHECK)
    f, i, v, u32 = ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32
    lib.hc_svf_logw.restype = f
    lib.hc_svf_logw.argtypes = [f, f, f, FP, f]
    lib.hc_svf_move.restype = f
    lib.hc_svf_move.argtypes = [f, FP, f, f]
    lib.hc_svf_pair_logw.restype = f
    lib.hc_svf_pair_logw.argtypes = [f, f, f, f, FP, f, FP]
    lib.hc_svf_filter_step.restype = ctypes.c_uint64
    lib.hc_svf_filter_step.argtypes = [v, i, FP, f, f, f, v, u32, v, v, v, v, FP]
    lib.hc_svf_draw.restype = i
    lib.hc_svf_draw.argtypes = [v, i, FP, f, i, f, f, f, u32, v, FP]
    lib.hc_sim_step.restype = None
    lib.hc_sim_step.argtypes = [i, FP, FP, f, FP, FP]
    lib.vissm_host_trans.restype = None
    lib.vissm_host_trans.argtypes = [i, FP, FP, FP, f, FP]
    return lib


def _p(a):
    return a.ctypes.data_as(FP)


def _bar(ref64, ref32):
    """The project's bar for a batch of values: 8 * max(e32, 2^-20 * mean |value|), e32 the largest deviation of the
    same formulas in numpy float32."""
    e32 = float(np.max(np.abs(ref32 - ref64)))
    return 8.0 * max(e32, 2.0 ** -20 * float(np.mean(np.abs(ref64)))), e32


def _points(rng, dt):
    """States around the SV config's range (h in [-12, -3]), observations around 1 .. 15 with steps of a few sd, and
    theta within 0.2 of viforssms_amd.sv.PARAM_INIT."""
    th = (np.asarray(R.PARAM_INIT) + rng.uniform(-0.2, 0.2, (NPTS, 4))).astype(np.float32)
    h = rng.uniform(-12.0, -3.0, NPTS).astype(np.float32)
    y0 = (rng.uniform(1.0, 15.0, NPTS) * rng.choice([-1.0, 1.0], NPTS)).astype(np.float32)
    sd = math.sqrt(dt) * np.abs(y0) * np.exp(0.5 * h.astype(np.float64))
    y1 = (y0 + sd * rng.uniform(-3.0, 3.0, NPTS)).astype(np.float32)
    y2 = (y1 + math.sqrt(dt) * np.abs(y1) * np.exp(0.5 * h.astype(np.float64)) * rng.uniform(-3.0, 3.0, NPTS)
          ).astype(np.float32)
    return th, h, y0, y1, y2


@pytest.mark.parametrize("dt", [1.0, 0.1])
def test_weight_and_move_match_float64(hc, dt):
    rng = np.random.default_rng(7 + int(10 * dt))
    th, h, y0, y1, _ = _points(rng, dt)
    nn = rng.standard_normal(NPTS).astype(np.float32)
    lw = np.array([hc.hc_svf_logw(h[i], y0[i], y1[i], _p(th[i]), dt) for i in range(NPTS)], np.float64)
    mv = np.array([hc.hc_svf_move(h[i], _p(th[i]), dt, nn[i]) for i in range(NPTS)], np.float32)
    lw64 = np.array([R.state_logw(np.float64(h[i]), y0[i], y1[i], th[i].astype(np.float64), dt) for i in range(NPTS)])
    lw32 = np.array([R.state_logw(h[i], y0[i], y1[i], th[i], dt, np.float32) for i in range(NPTS)], np.float64)
    bar, e32 = _bar(lw64, lw32)
    assert np.isfinite(lw).all() and np.all(np.abs(lw - lw64) <= bar), (float(np.max(np.abs(lw - lw64))), bar, e32)
    mv64 = R.h_step(h.astype(np.float64), th.astype(np.float64), dt, nn.astype(np.float64))
    mv32 = R.h_step(h, th, dt, nn, np.float32).astype(np.float64)
    bar, e32 = _bar(mv64, mv32)
    assert np.all(np.abs(mv - mv64) <= bar), (float(np.max(np.abs(mv - mv64))), bar, e32)
    # the move is sim::em_step<SV>'s second coordinate, bit for bit, whatever the first coordinate and its normal are
    for i in range(NPTS):
        x = np.array([y0[i], h[i]], np.float32)
        n2 = np.array([rng.standard_normal(), nn[i]], np.float32)
        out = np.zeros(2, np.float32)
        hc.hc_sim_step(SU.SV, _p(x), _p(np.concatenate([th[i], [0]]).astype(np.float32)), dt, _p(n2), _p(out))
        assert out[1:].view(np.int32)[0] == mv[i:i + 1].view(np.int32)[0], i
    # dead particles
    th0 = np.asarray(R.PARAM_INIT, np.float32)
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert hc.hc_svf_logw(bad, 1.0, 1.1, _p(th0), dt) == -math.inf
        assert math.isnan(hc.hc_svf_move(bad, _p(th0), dt, 0.3))
    assert math.isnan(hc.hc_svf_move(3.3e38, _p(np.array([0, 3.3e38, -100, 0], np.float32)), dt, 0.0))   # overflow dies


@pytest.mark.parametrize("dt", [1.0, 0.1])
def test_pair_logw_is_transition_plus_weight(hc, dt):
    """pair_logw + dropped_const = log f(xt | h) + state_logw(h, y_next, y_next2) in float64, and = the lp of the full
    SV transition em::sv_trans from (y_next, h) to (y_next2, xt), which factorises into exactly these two."""
    rng = np.random.default_rng(17 + int(10 * dt))
    th, h, _, y1, y2 = _points(rng, dt)
    xt = (R.h_mean(h.astype(np.float64), th.astype(np.float64), dt)
          + math.sqrt(dt) * np.exp(th[:, 3].astype(np.float64)) * rng.uniform(-4.0, 4.0, NPTS)).astype(np.float32)
    got, full = np.zeros(NPTS), np.zeros(NPTS)
    for i in range(NPTS):
        dropped = ctypes.c_float(0.0)
        lw = hc.hc_svf_pair_logw(h[i], xt[i], y1[i], y2[i], _p(th[i]), dt, ctypes.byref(dropped))
        want_drop = -math.log(math.sqrt(dt) * math.exp(float(th[i, 3]))) - PR.HALF_LOG_2PI
        assert abs(dropped.value - want_drop) <= 4e-6 * max(1.0, abs(want_drop))
        got[i] = float(np.float32(lw) + np.float32(dropped.value))
        out = np.zeros(10, np.float32)
        hc.vissm_host_trans(SU.SV, _p(np.array([y1[i], h[i]], np.float32)), _p(np.array([y2[i], xt[i]], np.float32)),
                            _p(np.concatenate([th[i], [0]]).astype(np.float32)), dt, _p(out))
        full[i] = out[0]
    f64 = lambda a: a.astype(np.float64)
    r64 = np.array([R.backward_logw(np.float64(h[i]), np.float64(xt[i]), f64(th[i]), dt, y1[i], y2[i])
                    for i in range(NPTS)])
    r32 = np.array([R.backward_logw(h[i], xt[i], th[i], dt, y1[i], y2[i], np.float32) for i in range(NPTS)], np.float64)
    bar, e32 = _bar(r64, r32)
    assert np.isfinite(got).all() and np.all(np.abs(got - r64) <= bar), (float(np.max(np.abs(got - r64))), bar, e32)
    assert np.all(np.abs(full - r64) <= bar)
    assert np.all(np.abs(got - full) <= 2.0 * bar)
    dropped = ctypes.c_float(0.0)
    th0 = np.asarray(R.PARAM_INIT, np.float32)
    assert math.isnan(hc.hc_svf_pair_logw(float("nan"), -8.0, 1.0, 1.1, _p(th0), dt, ctypes.byref(dropped)))
    assert math.isnan(hc.hc_svf_pair_logw(-8.0, float("nan"), 1.0, 1.1, _p(th0), dt, ctypes.byref(dropped)))


def test_serial_filter_step(hc):
    """One step of 64 particles, every fifth dead, run serially by the host build: the weights within the q bar of
    tests/test_gpu_particle.py of the float64 weights, the ancestors exactly the Python-int resampling of its own
    weights, each new h the bitwise move of its ancestor's."""
    n, dt = 64, 1.0
    rng = np.random.default_rng(71)
    th = np.asarray(R.PARAM_INIT, np.float32)
    h = rng.uniform(-10.0, -6.0, n).astype(np.float32)
    h[::5] = np.nan
    nn = rng.standard_normal(n).astype(np.float32)
    y0, y1 = np.float32(5.25), np.float32(5.31)
    ho, q = np.zeros(n, np.float32), np.zeros(n, np.uint64)
    anc, C, m = np.zeros(n, np.int32), np.zeros(n, np.uint64), ctypes.c_float(0.0)
    U = 0x5A5A5A
    W = hc.hc_svf_filter_step(h.ctypes.data, n, _p(th), dt, y0, y1, nn.ctypes.data, U, ho.ctypes.data, q.ctypes.data,
                              anc.ctypes.data, C.ctypes.data, ctypes.byref(m))
    want_anc, Wp = PR.systematic_ints(q, U)
    assert W == Wp > 0 and anc.tolist() == want_anc and int(q.max()) == 1 << 40 and not q[::5].any()
    alive, lw64, m64, qref = R.weigh(h.astype(np.float64), y0, y1, th.astype(np.float64), dt)
    live = np.where(alive)[0]
    lw32 = R.state_logw(h[live], y0, y1, th, dt, np.float32).astype(np.float64)
    d = 8.0 * max(float(np.max(np.abs(lw32 - lw64[live]))), 2.0 ** -20 * float(np.mean(np.abs(lw64[live]))))
    qr = qref.astype(np.float64)
    tol = qr * (math.expm1(2.0 * d) + (np.abs(np.where(alive, lw64, m64) - m64) + 2.0) * 2.0 ** -23) + 1.0
    assert np.all(np.abs(q.astype(np.float64) - qr) <= tol)
    for j in range(n):
        want = np.float32(hc.hc_svf_move(h[anc[j]], _p(th), dt, nn[j]))
        assert np.isfinite(ho[j]) and ho[j:j + 1].view(np.int32)[0] == np.array([want]).view(np.int32)[0], j
    h[:] = np.nan                                        # no live particle: W = 0, all NaN
    assert hc.hc_svf_filter_step(h.ctypes.data, n, _p(th), dt, y0, y1, nn.ctypes.data, U, ho.ctypes.data,
                                 q.ctypes.data, anc.ctypes.data, C.ctypes.data, ctypes.byref(m)) == 0
    assert np.isnan(ho).all() and not q.any()
    h[:] = -8.0                                          # y_prev = 0: every weight is NaN, the filter dies
    assert hc.hc_svf_filter_step(h.ctypes.data, n, _p(th), dt, 0.0, y1, nn.ctypes.data, U, ho.ctypes.data,
                                 q.ctypes.data, anc.ctypes.data, C.ctypes.data, ctypes.byref(m)) == 0


def test_serial_backward_draw(hc):
    """One backward draw over 128 particles, every fourth dead: the selection is the Python-int one of the traced
    weights, the weights lie within the q bar of the float64 ones; the terminal rule is uniform over the live
    particles; a NaN target and a column without live particles give -1."""
    n, dt = 128, 1.0
    rng = np.random.default_rng(73)
    th = np.asarray(R.PARAM_INIT, np.float32)
    h = rng.uniform(-10.0, -6.0, n).astype(np.float32)
    h[1::4] = np.nan
    y1, y2 = np.float32(5.25), np.float32(5.31)
    q, m = np.zeros(n, np.uint64), ctypes.c_float(0.0)
    for U in (0, 0x12345678, 0xFFFFFFFF):
        xt = np.float32(-8.3)
        idx = hc.hc_svf_draw(h.ctypes.data, n, _p(th), dt, 1, xt, y1, y2, U, q.ctypes.data, ctypes.byref(m))
        want, W, _ = PS.select_ints(q, U)
        assert idx == want and W > 0 and idx % 4 != 1 and int(q.max()) == 1 << 40 and not q[1::4].any()
        alive, lw64, m64, qref, _ = R.backward_draw(h.astype(np.float64), np.array([xt], np.float64),
                                                    th.astype(np.float64), dt, y1, y2, np.array([U], np.uint64))
        live = np.where(alive)[0]
        lw32 = R.backward_logw(h[live], xt, th, dt, y1, y2, np.float32).astype(np.float64)
        d = 8.0 * max(float(np.max(np.abs(lw32 - lw64[0, live]))), 2.0 ** -20 * float(np.mean(np.abs(lw64[0, live]))))
        qr = qref[0].astype(np.float64)
        gap = np.abs(np.where(alive, lw64[0], m64[0]) - m64[0])
        tol = qr * (math.expm1(2.0 * d) + (gap + 2.0) * 2.0 ** -23) + 1.0
        assert np.all(np.abs(q.astype(np.float64) - qr) <= tol)
        idx = hc.hc_svf_draw(h.ctypes.data, n, _p(th), dt, 0, 0.0, 0.0, 0.0, U, q.ctypes.data, ctypes.byref(m))
        assert np.array_equal(q, np.where(np.arange(n) % 4 == 1, 0, 1 << 40).astype(np.uint64))
        assert idx == PS.select_ints(q, U)[0] and idx % 4 != 1 and m.value == 0.0
        assert hc.hc_svf_draw(h.ctypes.data, n, _p(th), dt, 1, float("nan"), y1, y2, U, q.ctypes.data,
                              ctypes.byref(m)) == -1
    h[:] = np.nan
    for have_next in (0, 1):
        assert hc.hc_svf_draw(h.ctypes.data, n, _p(th), dt, have_next, -8.0, y1, y2, 9, q.ctypes.data,
                              ctypes.byref(m)) == -1


# ----------------------------------------------------------------------------------------------------------------
# refusals: host arithmetic before any GPU call
# ----------------------------------------------------------------------------------------------------------------
def test_filter_entry_refuses_without_gpu():
    from viforssms_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    P = ctypes.addressof(buf)
    names = ["theta", "x_start", "obs", "loglik_in", "loglik", "ll_inc", "ess", "state_end", "cloud", "q_trace",
             "anc_trace"]

    def call(desc, **null):
        ptrs = [None if null.get(n) else P for n in names]
        return lib.vissm_sv_filter(ctypes.byref(desc) if desc is not None else None, 1, 0, *ptrs, None)

    good = lambda **kw: _lib.PfDesc(**{**dict(model=_lib.MODEL_SV, K=0, N=64, H=4, t0=0, T_total=4, dt=1.0,
                                              obs_std=0.0), **kw})
    assert call(good()) == 0
    assert call(good(), loglik_in=True, cloud=True, q_trace=True, anc_trace=True) == 0
    for sd in (0.0, -1.0, float("nan"), float("inf"), 5.0):          # obs_std is ignored
        assert call(good(obs_std=sd)) == 0, sd
    assert call(None) == -1 and b"null descriptor" in lib.vissm_last_error()
    for model in (_lib.MODEL_AR, _lib.MODEL_LV, _lib.MODEL_FHN, 7, -1):
        assert call(good(model=model)) == -1 and b"SV" in lib.vissm_last_error()
    for n in (0, 1, 32, 63, 96, 100, 2048, -64):
        assert call(good(N=n)) == -1, n
        assert b"particles" in lib.vissm_last_error()
    for name in ("theta", "x_start", "loglik", "state_end", "obs", "ll_inc", "ess"):
        assert call(good(), **{name: True}) == -1, name
        assert b"null pointer" in lib.vissm_last_error()
    assert call(good(H=0), obs=True, ll_inc=True, ess=True) == 0
    for kw in (dict(K=-1), dict(H=-1), dict(t0=-1), dict(T_total=-1)):
        assert call(good(**kw)) == -1, kw
    assert call(good(t0=2, H=3, T_total=4)) == -1 and call(good(t0=2, H=2, T_total=4)) == 0
    big = 2 ** 31 - 1
    assert call(good(t0=big - 3, H=3, T_total=big)) == 0
    assert call(good(t0=big, H=big, T_total=big)) == -1 and b"2^31" in lib.vissm_last_error()
    assert call(good(K=2 ** 21, N=1024)) == -1 and b"K N" in lib.vissm_last_error()
    for dt in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert call(good(dt=dt)) == -1, dt
        assert b"dt" in lib.vissm_last_error()
    assert call(good(dt=1e-30)) == 0 and call(good(dt=3e38)) == 0
    want = {64: 4 * 64 * 64, 128: 4 * 128 * 64, 256: 4 * 256 * 64, 512: 4 * 512 * 64, 1024: 4 * 1024 * 32}
    for n in _lib.PF_PARTICLES:
        depth = 64 if n <= 512 else 32
        assert lib.vissm_sv_filter_lds_bytes(n) == want[n] + 12 * n + 8 * depth + 320
        assert lib.vissm_sv_filter_lds_bytes(n) <= 160 * 1024
        assert lib.vissm_sv_filter_lds_bytes(n) == lib.vissm_particle_filter_lds_bytes(_lib.MODEL_AR, n)
    for n in (0, 1, 63, 96, 2048, -64):
        assert lib.vissm_sv_filter_lds_bytes(n) == 0
    # the existing entries still refuse SV
    d = good()
    assert lib.vissm_particle_filter(ctypes.byref(d), 1, 0, *([P] * 12), None) == -1 and b"SV" in lib.vissm_last_error()
    assert lib.vissm_particle_filter_lds_bytes(_lib.MODEL_SV, 64) == 0


def test_smooth_entry_refuses_without_gpu():
    from viforssms_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    P = ctypes.addressof(buf)

    def call(desc, T_total=8, **null):
        g = lambda n: None if null.get(n) else P
        return lib.vissm_sv_smooth(ctypes.byref(desc) if desc is not None else None, 1, 0, g("theta"), g("cloud"),
                                   g("obs"), T_total, g("x_next"), g("paths"), g("x_first"), g("idx"), g("q_trace"),
                                   None)

    good = lambda **kw: _lib.PsDesc(**{**dict(model=_lib.MODEL_SV, K=0, N=128, M=64, H=4, t0=0, dt=1.0), **kw})
    assert call(good()) == 0 and call(good(), x_next=True, idx=True, q_trace=True) == 0
    assert call(None) == -1
    for model in (_lib.MODEL_AR, _lib.MODEL_LV, _lib.MODEL_FHN, 9, -1):
        assert call(good(model=model)) == -1 and b"SV" in lib.vissm_last_error()
    for n in (0, 32, 96, 2048):
        assert call(good(N=n)) == -1 and b"particles" in lib.vissm_last_error()
    for m in (0, 32, 96, 256, -64):
        assert call(good(M=m)) == -1 and b"trajectories" in lib.vissm_last_error()
    for kw in (dict(K=-1), dict(K=65536), dict(H=0), dict(H=-1), dict(t0=-1)):
        assert call(good(**kw)) == -1, kw
    assert call(good(), T_total=-1) == -1
    for name in ("theta", "cloud", "obs", "paths", "x_first"):
        assert call(good(), **{name: True}) == -1 and b"null pointer" in lib.vissm_last_error()
    # every column with a next state reads y[ca + 2]: t0 + H + 1 <= T_total with x_next, t0 + H without
    # (x_next=True leaves x_next NULL)
    assert call(good(t0=4, H=4), T_total=8, x_next=True) == 0
    assert call(good(t0=4, H=4), T_total=8) == -1 and b"next state" in lib.vissm_last_error()
    assert call(good(t0=3, H=4), T_total=8) == 0
    assert call(good(t0=5, H=4), T_total=8, x_next=True) == -1
    big = 2 ** 31 - 1
    assert call(good(t0=big - 1, H=1), T_total=big, x_next=True) == 0
    assert call(good(t0=big, H=1), T_total=big, x_next=True) == -1 and b"2^31" in lib.vissm_last_error()
    for dt in (0.0, -1.0, float("nan"), float("inf")):
        assert call(good(dt=dt)) == -1 and b"dt" in lib.vissm_last_error()
    depth = {64: 32, 128: 32, 256: 16, 512: 8, 1024: 4}
    for n in _lib.PF_PARTICLES:
        for m in (64, n):
            want = 4 * n * depth[n] + 8 * n + 512 * depth[n] + 768 * min(4, n // 64) + 512
            assert lib.vissm_sv_smooth_lds_bytes(n, m) == want <= 64 * 1024
    assert lib.vissm_sv_smooth_lds_bytes(96, 64) == 0 and lib.vissm_sv_smooth_lds_bytes(128, 256) == 0
    assert lib.vissm_sv_smooth_lds_bytes(128, 96) == 0 and lib.vissm_sv_smooth_lds_bytes(128, 32) == 0
    d = _lib.PsDesc(model=_lib.MODEL_SV, K=0, N=128, M=64, H=4, t0=0, dt=1.0)
    assert lib.vissm_particle_smooth(ctypes.byref(d), 1, 0, *([P] * 7), None) == -1 and b"SV" in lib.vissm_last_error()
    assert lib.vissm_particle_smooth_lds_bytes(_lib.MODEL_SV, 128, 64) == 0


def test_python_refusals_without_gpu():
    import torch
    from viforssms_amd import _lib, ops
    th, z = torch.zeros(1, 4), torch.zeros(9)
    with pytest.raises(_lib.VissmError, match="particles"):
        ops.sv_filter(th, z[:1], z, 1.0, 96, 1, 0)
    for dt in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.VissmError, match="dt"):
            ops.sv_filter(th, z[:1], z, dt, 64, 1, 0)
    with pytest.raises(_lib.VissmError, match="GPU only"):
        ops.sv_filter(th, z[:1], z, 1.0, 64, 1, 0)
    with pytest.raises(_lib.VissmError, match="GPU only"):
        ops.sv_smooth(th, torch.zeros(64, 1, 4), z, 1.0, 64, 1, 0)
    assert _lib.SIGNATURES["vissm_sv_filter"][1][0] is _lib.SIGNATURES["vissm_particle_filter"][1][0]   # one descriptor


def test_cli_options():
    from viforssms_amd import sv
    with pytest.raises(SystemExit):
        sv.run(["--filter", "four", "64", "f.npz"])
    with pytest.raises(SystemExit):
        sv.run(["--smooth", "4", "64", "f.npz"])


# ----------------------------------------------------------------------------------------------------------------
# the statistical bars, for the reference alone
# ----------------------------------------------------------------------------------------------------------------
def test_grid_truth_and_fixture():
    """The two grid sizes agree to 1e-6 (fixture_truth asserts it); a grid pass run here at a third size reproduces
    the stored log-evidence and smoothing moments; the stored series is what the generator's seed simulates."""
    L, ms, sds = R.fixture_truth()
    z = R.fixture()
    assert z["y"].shape == (R.FIX_T + 1,) and z["y"].dtype == np.float32 and np.isfinite(z["y"]).all()
    assert not np.any(z["y"][:-1] == 0) and z["ref_logliks"].shape == (R.FIX_K,)
    y, _ = R.simulate_series(R.FIX_T, R.PARAM_INIT, R.FIX_DT, R.FIX_H0, R.FIX_Y0,
                             np.random.default_rng(int(z["seed"])))
    assert np.allclose(y, z["y"], rtol=1e-6)
    g = R.grid_pass(R.PARAM_INIT, R.FIX_H0, z["y"].astype(np.float64), R.FIX_DT, 1201)
    assert abs(g["loglik"] - L) <= 1e-6 and np.max(np.abs(g["ms"] - ms)) <= 1e-6
    assert np.max(np.abs(g["sds"] - sds)) <= 1e-6


def test_reference_meets_its_own_bars():
    """K = 1024 filters of N = 256: two seeds of the numpy filter against each other, against the fixture's stored
    estimates and against the grid value (pf_ref.stat_bars, K = 256 against K_r = 1024)."""
    L, _, _ = R.fixture_truth()
    a, b, stored = R.reference_logliks(1), R.reference_logliks(2), R.fixture()["ref_logliks"]
    assert np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(stored).all()
    for small, large in ((a[:256], b), (b[:256], a), (a[:256], stored), (stored[:256], b)):
        mu, s, mu_r, s_r = small.mean(), small.std(ddof=1), large.mean(), large.std(ddof=1)
        bars = PR.stat_bars(mu, s, small.size, mu_r, s_r, large.size, L)
        print(f"L {L:.4f} mu {mu:.4f} s {s:.4f} mu_r {mu_r:.4f} s_r {s_r:.4f} {bars}")
        assert all(bars.values()), bars


def test_reference_smoother_matches_the_grid_smoother():
    """The numpy FFBSi (64 filters of N = 256, M = 64 trajectories each) against the grid smoother: bars (b) and (c)
    of tests/ps_ref.py -- the mean within 0.2 smoothing sd and the pooled sd within 0.85 .. 1.15 at every step."""
    _, ms, sds = R.fixture_truth()
    paths = R.reference_paths(5, K=64)
    assert np.isfinite(paths).all()
    mean, _, sd = PS.stat_moments(paths)
    bars = R.smooth_bars(mean, sd, ms, sds)
    print(f"(b) {bars['b'][1]:.4f} sd (c) {bars['c'][1][0]:.4f} .. {bars['c'][1][1]:.4f}")
    assert bars["b"][0] and bars["c"][0], bars
