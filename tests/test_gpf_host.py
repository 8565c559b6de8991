"""The fully adapted particle filter without a GPU: csrc/gp_math.hpp (the code the kernel runs, built for the host
in libvissm_hostcheck.so) against the numpy.linalg reference of tests/gpf_ref.py on the general formulas; its
identities and its clamp; one serial filter step; the library's refusals, which are host arithmetic; the unchanged
ABI; and the statistical bars of tests/test_gpu_adapted.py for the numpy reference alone."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import gpf_ref as GR
from tests import pf_ref as PR
from tests import sim_util as SU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK = os.path.join(ROOT, "viforssms_amd", "libvissm_hostcheck.so")
FP = ctypes.POINTER(ctypes.c_float)
RELS = (0.05, 0.3, 1.0, 30.0, 1e3)       # obs_std in units of the observed coordinate's transition sd
NPTS = 64


@pytest.fixture(scope="module")
def hc():
    lib = ctypes.CDLL(HOSTCHECK)
    f, i, v = ctypes.c_float, ctypes.c_int, ctypes.c_void_p
    lib.hc_gp_moments.restype = None
    lib.hc_gp_moments.argtypes = [i, FP, FP, f, FP]
    lib.hc_gp_logw.restype = f
    lib.hc_gp_logw.argtypes = [i, FP, FP, f, FP, FP, f]
    lib.hc_gp_cond.restype = None
    lib.hc_gp_cond.argtypes = [i, FP, FP, f, FP, FP, f, FP]
    lib.hc_gp_step.restype = None
    lib.hc_gp_step.argtypes = [i, FP, FP, f, FP, FP, f, FP, FP]
    lib.hc_gp_l11.restype = f
    lib.hc_gp_l11.argtypes = [f, f]
    lib.hc_gp_filter_step.restype = ctypes.c_uint64
    lib.hc_gp_filter_step.argtypes = [i, v, i, FP, f, FP, FP, f, v, ctypes.c_uint32, v, v, v, v, FP]
    lib.hc_sim_step.restype = None
    lib.hc_sim_step.argtypes = [i, FP, FP, f, FP, FP]
    return lib


def _p(a):
    return a.ctypes.data_as(FP)


def _pad(a, n):
    out = np.zeros(n, np.float32)
    out[:len(a)] = a
    return out


def _points(model, rng, n=NPTS):
    """n states and thetas around the generators' true values (tests/test_sim_host.py's range), and normals."""
    S, P = SU.S_OF[model], SU.P_OF[model]
    x = (np.asarray(SU.TRUE_X[model]) * rng.uniform(0.7, 1.3, (n, S))).astype(np.float32)
    th = (np.asarray(SU.TRUE_THETA[model]) + rng.uniform(-0.1, 0.1, (n, P))).astype(np.float32)
    return x, th, rng.standard_normal((n, 2)).astype(np.float32)


def _header(hc, model, x, th, dt, y, b, obs_std, nn):
    """logw [n], m [n, S], L [n, S, S], step [n, S] of the header for each point, R = fp32 obs_std^2."""
    n, S = x.shape
    R = float(np.float32(obs_std) * np.float32(obs_std))
    lw, m, L, st = np.zeros(n), np.zeros((n, S)), np.zeros((n, S, S)), np.zeros((n, S))
    for i in range(n):
        xi, thi, out, so = _pad(x[i], 2), _pad(th[i], 5), np.zeros(5, np.float32), np.zeros(2, np.float32)
        yi, bi = _pad(y[i], 2), _pad(b, 2)
        lw[i] = hc.hc_gp_logw(model, _p(xi), _p(thi), dt, _p(yi), _p(bi), R)
        hc.hc_gp_cond(model, _p(xi), _p(thi), dt, _p(yi), _p(bi), R, _p(out))
        hc.hc_gp_step(model, _p(xi), _p(thi), dt, _p(yi), _p(bi), R, _p(nn[i].copy()), _p(so))
        m[i] = out[:S]
        L[i, 0, 0] = out[2]
        if S == 2:
            L[i, 1, 0], L[i, 1, 1] = out[3], out[4]
        st[i] = so[:S]
    return lw, m, L, st


def _reference(model, x, th, dt, y, b, obs_std, nn, dtype):
    """The same from tests/gpf_ref.py in `dtype`, one point at a time (each point has its own y), plus P."""
    n, S = x.shape
    lw, m, L, P, st = np.zeros(n), np.zeros((n, S)), np.zeros((n, S, S)), np.zeros((n, S, S)), np.zeros((n, S))
    for i in range(n):
        xi, thi = x[i].astype(dtype), th[i].astype(dtype)
        mu, Sg = GR.moments(model, xi, thi, dt)
        lw[i] = GR.predictive_logw(mu, Sg, y[i], b, dtype(obs_std))
        m[i], L[i], P[i] = GR.conditional(mu, Sg, y[i], b, dtype(obs_std))
        st[i] = GR.propagate(model, xi, thi, dt, y[i], b, dtype(obs_std), nn[i].astype(dtype))
    return lw, m, L, P, st


def _case(model, b, rel, rng):
    """Points, an obs_std of `rel` transition sd of the first observed coordinate at the true state, and per-point
    observations within two predictive sd of the predictive mean (NaN filler where unobserved: never read)."""
    S, dt = SU.S_OF[model], SU.DT[model]
    x, th, nn = _points(model, rng)
    _, Sg0 = GR.moments(model, np.asarray(SU.TRUE_X[model], np.float64), np.asarray(SU.TRUE_THETA[model]), dt)
    d0 = GR.observed(b)[0]
    obs_std = float(np.float32(rel * math.sqrt(Sg0[d0, d0])))
    mu, Sg = GR.moments(model, x.astype(np.float64), th.astype(np.float64), dt)
    sd = np.sqrt(np.diagonal(Sg, axis1=-2, axis2=-1) + obs_std ** 2)
    y = (mu + sd * rng.uniform(-2.0, 2.0, (NPTS, S))).astype(np.float32)
    y[:, [d for d in range(S) if b[d] == 0]] = np.nan
    return x, th, nn, obs_std, y


def _bar(ref64, ref32):
    """The project's bar for a batch of values: 8 * max(e32, 2^-20 * mean |value|), e32 the largest deviation of the
    same formulas in numpy float32."""
    e32 = float(np.max(np.abs(ref32 - ref64)))
    return 8.0 * max(e32, 2.0 ** -20 * float(np.mean(np.abs(ref64)))), e32


MASKS = [(SU.AR, (1,)), (SU.LV, (1, 1)), (SU.LV, (1, 0)), (SU.LV, (0, 1)), (SU.FHN, (1, 1)), (SU.FHN, (1, 0)),
         (SU.FHN, (0, 1))]


@pytest.mark.parametrize("model,mask", MASKS)
def test_header_matches_the_linalg_reference(hc, model, mask):
    """logw, m, L and the step of gp_math.hpp against numpy.linalg in float64, within 8 * max(e32, 2^-20 mean
    |value|) per quantity and coordinate; L L^T = Sigma - K Sigma_O. against the float64 P in the same form."""
    S, dt = SU.S_OF[model], SU.DT[model]
    rng = np.random.default_rng(500 + 10 * model + sum(m << i for i, m in enumerate(mask)))
    worst = {}
    for rel in RELS:
        x, th, nn, obs_std, y = _case(model, mask, rel, rng)
        lw, m, L, st = _header(hc, model, x, th, dt, y, mask, obs_std, nn)
        lw64, m64, L64, P64, st64 = _reference(model, x, th, dt, y, mask, obs_std, nn, np.float64)
        lw32, m32, L32, _, st32 = _reference(model, x, th, dt, y, mask, obs_std, nn, np.float32)
        assert np.isfinite(lw).all() and np.isfinite(m).all() and np.isfinite(L).all() and np.isfinite(st).all()
        checks = [("logw", lw, lw64, lw32)]
        for d in range(S):
            checks.append((f"m{d}", m[:, d], m64[:, d], m32[:, d]))
            checks.append((f"x{d}", st[:, d], st64[:, d], st32[:, d]))
            for e in range(d + 1):
                checks.append((f"l{d}{e}", L[:, d, e], L64[:, d, e], L32[:, d, e]))
        LLt, LLt32 = L @ np.swapaxes(L, 1, 2), L32 @ np.swapaxes(L32, 1, 2)
        for d in range(S):
            for e in range(d + 1):
                checks.append((f"p{d}{e}", LLt[:, d, e], P64[:, d, e], LLt32[:, d, e]))
        for name, got, r64, r32 in checks:
            bar, e32 = _bar(r64, r32)
            share = float(np.max(np.abs(got - r64))) / bar if bar > 0 else 0.0
            worst[name] = max(worst.get(name, 0.0), share)
            assert np.all(np.abs(got - r64) <= bar), (model, mask, rel, name, share, e32)
        if S == 2:
            assert np.all(L[:, 0, 1] == 0.0)
    print(f"model {model} mask {mask}: largest shares of the bars "
          + " ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


@pytest.mark.parametrize("model,mask", MASKS)
def test_vague_observation_gives_the_plain_step(hc, model, mask):
    """At obs_std = 1000 transition sd the gain g = max Sigma_dd / (Sigma_dd + R) is about 1e-6, so the conditional
    is the transition up to g: |m - mu| <= g |y_O - mu_O| summed over the observed coordinates times the covariance
    ratio, and L differs from chol(Sigma) by a factor within g.  With a four-fold margin for the cross terms and 16
    fp32 ulp of the terms for rounding: |x'_adapted - x'_em| <= 4 g (sum |r| + sum |L n|) + 16 * 2^-24 sum |terms|."""
    S, dt = SU.S_OF[model], SU.DT[model]
    rng = np.random.default_rng(900 + model)
    x, th, nn, obs_std, y = _case(model, mask, 1e3, rng)
    _, _, _, st = _header(hc, model, x, th, dt, y, mask, obs_std, nn)
    mu, Sg = GR.moments(model, x.astype(np.float64), th.astype(np.float64), dt)
    R = obs_std ** 2
    for i in range(NPTS):
        out = np.zeros(2, np.float32)
        hc.hc_sim_step(model, _p(_pad(x[i], 2)), _p(_pad(th[i], 5)), dt, _p(nn[i].copy()), _p(out))
        O = GR.observed(mask)
        g = max(Sg[i, d, d] / (Sg[i, d, d] + R) for d in range(S))
        r = sum(abs(float(y[i, d]) - mu[i, d]) for d in O)
        Ln = float(np.sum(np.abs(np.linalg.cholesky(Sg[i])) @ np.abs(nn[i, :S].astype(np.float64))))
        terms = float(np.sum(np.abs(mu[i]))) + Ln
        bound = 4.0 * g * (r + Ln) + 16.0 * 2.0 ** -24 * terms
        assert g < 2e-6
        assert np.all(np.abs(st[i] - out[:S].astype(np.float64)) <= bound), (model, mask, i, st[i], out[:S], bound)


def test_clamp(hc):
    """A P11 - l10^2 that rounds negative gives l11 = 0, not NaN; a NaN radicand (a dead particle) stays NaN."""
    assert hc.hc_gp_l11(1.0, 1.0000001) == 0.0
    assert hc.hc_gp_l11(1.0, float(np.nextafter(np.float32(1.0), np.float32(2.0)))) == 0.0
    assert hc.hc_gp_l11(0.0, 0.0) == 0.0 and hc.hc_gp_l11(4.0, 0.0) == 2.0 and hc.hc_gp_l11(25.0, 3.0) == 4.0
    assert math.isnan(hc.hc_gp_l11(float("nan"), 1.0)) and math.isnan(hc.hc_gp_l11(1.0, float("nan")))


@pytest.mark.parametrize("model,mask", [(SU.AR, (1,)), (SU.LV, (1, 1)), (SU.LV, (0, 1)), (SU.FHN, (1, 0))])
def test_serial_filter_step(hc, model, mask):
    """One adapted step of 64 particles, every fifth dead, run serially by the host build: the weights within the q
    bar of tests/test_gpu_particle.py of the float64 predictive weights, the ancestors exactly the Python-int
    resampling of its own weights, each new state within the state bar of the float64 draw from its ancestor."""
    S, P, dt, n = SU.S_OF[model], SU.P_OF[model], SU.DT[model], 64
    rng = np.random.default_rng(70 + model)
    x = (np.asarray(SU.TRUE_X[model]) * rng.uniform(0.8, 1.2, (n, S))).astype(np.float32)
    x[::5, 0] = np.nan
    th = np.asarray(SU.TRUE_THETA[model], np.float32)
    nn = rng.standard_normal((n, S)).astype(np.float32)
    b = _pad(np.asarray(mask, np.float32), 2)
    obs_std = {SU.AR: 1.0, SU.LV: 2.0, SU.FHN: 0.1}[model]
    y = _pad(np.asarray(SU.TRUE_X[model], np.float32) * 1.02, 2)
    xo, q = np.zeros((n, S), np.float32), np.zeros(n, np.uint64)
    anc, C, m = np.zeros(n, np.int32), np.zeros(n, np.uint64), ctypes.c_float(0.0)
    U = 0x5A5A5A
    W = hc.hc_gp_filter_step(model, x.ctypes.data, n, _p(_pad(th, 5)), dt, _p(y), _p(b), obs_std, nn.ctypes.data, U,
                             xo.ctypes.data, q.ctypes.data, anc.ctypes.data, C.ctypes.data, ctypes.byref(m))
    want_anc, Wp = PR.systematic_ints(q, U)
    assert W == Wp > 0 and anc.tolist() == want_anc and int(q.max()) == 1 << 40 and not q[::5].any()
    thn = np.tile(th, (n, 1))
    alive, lw64, m64, qref = GR.weigh(model, x.astype(np.float64), thn.astype(np.float64), dt, y[:S], mask, obs_std)
    live = np.where(alive)[0]
    mu32, Sg32 = GR.moments(model, x[live], thn[live], dt)
    lw32 = GR.predictive_logw(mu32, Sg32, y[:S], mask, np.float32(obs_std)).astype(np.float64)
    d = 8.0 * max(float(np.max(np.abs(lw32 - lw64[live]))), 2.0 ** -20 * float(np.mean(np.abs(lw64[live]))))
    qr = qref.astype(np.float64)
    tol = qr * (math.expm1(2.0 * d) + (np.abs(np.where(alive, lw64, m64) - m64) + 2.0) * 2.0 ** -23) + 1.0
    assert np.all(np.abs(q.astype(np.float64) - qr) <= tol)
    xa = x[anc]
    x64 = GR.propagate(model, xa.astype(np.float64), thn.astype(np.float64), dt, y[:S], mask, obs_std, nn)
    x32 = GR.propagate(model, xa, thn, dt, y[:S], mask, np.float32(obs_std), nn)
    e32 = float(np.max(np.abs(x32 - x64)))
    bar = 8.0 * np.maximum(e32, 2.0 ** -20 * np.mean(np.abs(x64), axis=0))
    assert np.isfinite(xo).all() and np.all(np.abs(xo - x64) <= bar), float(np.max(np.abs(xo - x64) / bar))
    # nothing observed: the forecast's step, slot for slot
    none = np.zeros(2, np.float32)
    hc.hc_gp_filter_step(model, x.ctypes.data, n, _p(_pad(th, 5)), dt, _p(y), _p(none), obs_std, nn.ctypes.data, U,
                         xo.ctypes.data, q.ctypes.data, anc.ctypes.data, C.ctypes.data, ctypes.byref(m))
    for i in range(n):
        out = np.zeros(2, np.float32)
        hc.hc_sim_step(model, _p(_pad(x[i], 2)), _p(_pad(th, 5)), dt, _p(_pad(nn[i], 2)), _p(out))
        want = out[:S] if SU.alive(model, out[:S]) else np.full(S, np.nan, np.float32)
        assert np.array_equal(xo[i], want, equal_nan=True), i
    assert anc.tolist() == list(range(n)) and not q.any()


def test_abi_is_unchanged():
    from viforssms_amd import _lib
    lib = ctypes.CDLL(HOSTCHECK)
    out = (ctypes.c_size_t * 2)()
    lib.vissm_host_abi_layout.restype = None
    lib.vissm_host_abi_layout(6, out)
    assert out[0] == ctypes.sizeof(_lib.PfDesc) == 32 and out[1] == _lib.PfDesc.obs_std.offset == 28
    assert [f[0] for f in _lib.PfDesc._fields_] == ["model", "K", "N", "H", "t0", "T_total", "dt", "obs_std"]
    a, b = _lib.SIGNATURES["vissm_particle_filter_adapted"], _lib.SIGNATURES["vissm_particle_filter"]
    assert a[0] is b[0] and a[1] == b[1]


def test_library_refuses_without_gpu():
    """Everything vissm_particle_filter refuses, and obs_std <= 0 or not finite: host arithmetic before any GPU call,
    so with every pointer a dummy a bad descriptor comes back VISSM_EINVAL and a good one with K = 0 is a no-op."""
    from viforssms_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    P = ctypes.addressof(buf)
    names = ["theta", "x_start", "obs", "obs_bin", "loglik_in", "loglik", "ll_inc", "ess", "state_end", "cloud",
             "q_trace", "anc_trace"]

    def call(desc, fn=lib.vissm_particle_filter_adapted, **null):
        ptrs = [None if null.get(n) else P for n in names]
        return fn(ctypes.byref(desc) if desc is not None else None, 1, 0, *ptrs, None)

    good = lambda **kw: _lib.PfDesc(**{**dict(model=_lib.MODEL_AR, K=0, N=64, H=4, t0=0, T_total=4, dt=1.0,
                                              obs_std=1.0), **kw})
    assert call(good()) == 0
    assert call(good(), loglik_in=True, cloud=True, q_trace=True, anc_trace=True) == 0
    for sd in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert call(good(obs_std=sd)) == -1, sd
        assert b"obs_std" in lib.vissm_last_error()
        assert call(good(obs_std=sd), fn=lib.vissm_particle_filter) == 0        # the bootstrap entry is as it was
    assert call(good(obs_std=1e-30)) == 0 and call(good(obs_std=3e38)) == 0
    for model in (_lib.MODEL_AR, _lib.MODEL_LV, _lib.MODEL_FHN):
        for n in _lib.PF_PARTICLES:
            assert lib.vissm_particle_filter_adapted_lds_bytes(model, n) == \
                lib.vissm_particle_filter_lds_bytes(model, n) > 0
    assert lib.vissm_particle_filter_adapted_lds_bytes(_lib.MODEL_LV, 1024) == 147904
    assert lib.vissm_particle_filter_adapted_lds_bytes(_lib.MODEL_SV, 64) == 0
    assert lib.vissm_particle_filter_adapted_lds_bytes(_lib.MODEL_AR, 96) == 0
    # the bootstrap entry's own list
    for n in (0, 1, 32, 63, 96, 100, 2048, -64):
        assert call(good(N=n)) == -1, n
        assert b"particles" in lib.vissm_last_error()
    assert call(good(model=_lib.MODEL_SV)) == -1 and b"SV" in lib.vissm_last_error()
    assert call(good(model=7)) == -1 and call(good(model=-1)) == -1
    assert call(None) == -1
    for name in ("theta", "x_start", "loglik", "state_end", "obs", "obs_bin", "ll_inc", "ess"):
        assert call(good(), **{name: True}) == -1, name
        assert b"null pointer" in lib.vissm_last_error()
    for kw in (dict(K=-1), dict(H=-1), dict(t0=-1), dict(T_total=-1)):
        assert call(good(**kw)) == -1, kw
    assert call(good(t0=2, H=3, T_total=4)) == -1
    big = 2 ** 31 - 1
    assert call(good(model=_lib.MODEL_LV, t0=2 ** 30, H=8, T_total=big)) == -1
    assert b"2^31" in lib.vissm_last_error()
    assert call(good(model=_lib.MODEL_LV, t0=2 ** 30 - 8, H=7, T_total=big)) == 0
    assert call(good(t0=big - 3, H=3, T_total=big)) == 0
    assert call(good(t0=big, H=big, T_total=big)) == -1
    assert call(good(K=2 ** 22, N=1024)) == -1


def test_python_refusals_without_gpu():
    """ops.particle_filter refuses an unknown proposal and a degenerate obs_std before it looks at a tensor."""
    import torch
    from viforssms_amd import _lib, ops
    z = torch.zeros(1, 3)
    with pytest.raises(_lib.VissmError, match="proposal"):
        ops.particle_filter(SU.AR, z, z, z, z, 1.0, 1.0, 64, 1, 0, proposal="optimal")
    for sd in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.VissmError, match="obs_std"):
            ops.particle_filter(SU.AR, z, z, z, z, 1.0, sd, 64, 1, 0, proposal="adapted")
    with pytest.raises(_lib.VissmError, match="GPU only"):
        ops.particle_filter(SU.AR, z, z, z, z, 1.0, 1.0, 64, 1, 0, proposal="adapted")


def test_cli_option():
    from viforssms_amd import config
    base = ["hyperparameters.txt"]
    assert config.handle_opts(base + ["--filter", "4", "64", "f.npz"]).filter_proposal == "bootstrap"
    assert config.handle_opts(base + ["--filter", "4", "64", "f.npz", "--filter-proposal", "adapted"]
                             ).filter_proposal == "adapted"
    assert config.handle_opts(base + ["--smooth", "4", "64", "64", "s.npz", "--filter-proposal", "adapted"]
                             ).filter_proposal == "adapted"
    assert config.handle_opts(base).filter_proposal == "bootstrap"
    for bad in (["--filter-proposal", "adapted"], ["--filter", "4", "64", "f.npz", "--filter-proposal", "optimal"]):
        with pytest.raises(SystemExit):
            config.handle_opts(base + bad)


# ----------------------------------------------------------------------------------------------------------------
# the statistical bars, for the reference alone
# ----------------------------------------------------------------------------------------------------------------
def test_reference_meets_its_own_bars_ar():
    """AR fixture, K = 1024, N = 256: two seeds of the numpy adapted filter against each other and against Kalman
    (pf_ref.stat_bars, K = 256 against K_r = 1024 and the two swapped), and the discriminating condition: the sd of
    the adapted estimates is at most a quarter of the bootstrap reference's (measured: 0.114 against 0.94, a ratio
    of 0.12, so the bar leaves a factor of two)."""
    L = PR.stat_kalman()
    a, b = GR.reference_logliks(1), GR.reference_logliks(2)
    boot = PR.reference_logliks(101)
    assert np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(boot).all()
    s_boot = boot.std(ddof=1)
    for small, large in ((a[:256], b), (b[:256], a)):
        mu, s, mu_r, s_r = small.mean(), small.std(ddof=1), large.mean(), large.std(ddof=1)
        bars = PR.stat_bars(mu, s, small.size, mu_r, s_r, large.size, L)
        print(f"L {L:.4f} mu {mu:.4f} s {s:.4f} mu_r {mu_r:.4f} s_r {s_r:.4f} s_boot {s_boot:.4f} {bars}")
        assert all(bars.values()), bars
        assert s <= 0.25 * s_boot and s_r <= 0.25 * s_boot


@pytest.mark.parametrize("model,obs_std,mask", GR.SMALL_CASES)
def test_reference_agrees_with_the_bootstrap_reference(model, obs_std, mask):
    """LV and FHN, T = 40, observed every fifth step, K = 256 filters of N = 256 per proposal: both estimate the same
    evidence, so -4 se <= mu_adapted - mu_bootstrap <= s_b^2 + 4 se (gpf_ref.jensen_bars)."""
    la = GR.small_logliks(model, obs_std, mask, "adapted")
    lb = GR.small_logliks(model, obs_std, mask, "bootstrap")
    assert np.isfinite(la).all() and np.isfinite(lb).all()
    r = GR.jensen_bars(la, lb)
    print(f"model {model} obs_std {obs_std} mask {mask}: adapted {r['mu_a']:.3f} sd {r['s_a']:.3f}, bootstrap "
          f"{r['mu_b']:.3f} sd {r['s_b']:.3f}, se {r['se']:.3f}")
    assert r["ok"], r
