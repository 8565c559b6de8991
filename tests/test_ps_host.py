"""The particle smoother without a GPU: csrc/ps_math.hpp (the code the kernel runs, built for the host in
libvissm_hostcheck.so) against Python big ints and float64; the library's refusals, which are host arithmetic; the RTS
smoother of tests/ps_ref.py against the dense Gaussian posterior; and the statistical bars of
tests/test_gpu_smooth.py for the numpy reference alone, two seeds against each other and against RTS."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import pf_ref as PR
from tests import ps_ref as PS
from tests import sim_util as SU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK = os.path.join(ROOT, "viforssms_amd", "libvissm_hostcheck.so")
UMAX = (1 << 32) - 1
ONE = 1 << 40


@pytest.fixture(scope="module")
def hc():
    lib = ctypes.CDLL(HOSTCHECK)
    V, F = ctypes.c_void_p, ctypes.c_float
    lib.hc_ps_pair_logw.restype = F
    lib.hc_ps_pair_logw.argtypes = [ctypes.c_int, V, V, V, F, V]
    lib.hc_ps_threshold.restype = ctypes.c_uint64
    lib.hc_ps_threshold.argtypes = [ctypes.c_uint32, ctypes.c_uint64]
    lib.hc_ps_select_u.restype = ctypes.c_uint32
    lib.hc_ps_select_u.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64]
    lib.hc_ps_select.restype = ctypes.c_int
    lib.hc_ps_select.argtypes = [V, ctypes.c_int, ctypes.c_uint32, V, V]
    lib.hc_ps_draw.restype = ctypes.c_int
    lib.hc_ps_draw.argtypes = [ctypes.c_int, V, ctypes.c_int, V, F, V, ctypes.c_uint32, V, V]
    lib.hc_ps_valid_m.restype = ctypes.c_int
    lib.hc_ps_valid_m.argtypes = [ctypes.c_int, ctypes.c_int]
    return lib


def _select(hc, q, U):
    q = np.ascontiguousarray(q, np.uint64)
    W, tau = ctypes.c_uint64(99), ctypes.c_uint64(99)
    idx = hc.hc_ps_select(q.ctypes.data, q.size, U, ctypes.addressof(W), ctypes.addressof(tau))
    return idx, W.value, tau.value


def _weight_cases(n, rng):
    """All-equal weights (W = N 2^40: 2^50 at N = 1024, and with U = j 2^32 / N every tau falls exactly on C_{j-1});
    one below; one live particle; runs of zeros; three unit weights behind N - 3 zeros; thirty e-folds."""
    full = np.full(n, ONE, np.uint64)
    below = full.copy()
    below[-1] -= np.uint64(1)
    one = np.zeros(n, np.uint64)
    one[n // 3] = ONE
    runs = rng.integers(0, ONE, n, dtype=np.uint64)
    runs[(np.arange(n) // 7) % 2 == 1] = 0
    runs[5] = ONE
    tail = np.zeros(n, np.uint64)
    tail[-3:] = 1
    spread = np.floor(np.exp(rng.uniform(-30.0, 0.0, n)) * ONE).astype(np.uint64)
    spread[0] = ONE
    return {"full": full, "below": below, "one": one, "runs": runs, "tail": tail, "spread": spread}


@pytest.mark.parametrize("n", [64, 1024])
def test_selection_matches_python_ints(hc, n):
    rng = np.random.default_rng(n)
    for name, q in _weight_cases(n, rng).items():
        for U in (0, 1, UMAX // 2, UMAX // 2 + 1, UMAX - 1, UMAX, (n // 2) << (32 - n.bit_length() + 1)):
            want, W, tau = PS.select_ints(q, U)
            idx, Wc, tc = _select(hc, q, U)
            assert (Wc, tc) == (W, tau) and tau < W, (name, U)
            assert idx == want and 0 <= idx < n and int(q[idx]) > 0, (name, U, idx, want)
            assert hc.hc_ps_threshold(U, W) == (U * W) >> 32
            v_idx, v_W = PS.select_u64(q[None, :], np.asarray([U], np.uint64))      # the reference's vectorised form
            assert int(v_idx[0]) == want and int(v_W[0]) == W, (name, U)
    # tau exactly on a C_i: the particle whose cumulative sum equals tau is passed over (C_i <= tau counts it)
    q = np.full(n, ONE, np.uint64)
    for j in (1, n // 2, n - 1):
        U = j * (1 << 32) // n
        assert (U * n * ONE) >> 32 == j * ONE and _select(hc, q, U)[0] == j
    assert _select(hc, q, 0)[0] == 0 and _select(hc, q, UMAX)[0] == n - 1
    # W = 2^50, the largest sum N = 1024 reaches
    assert hc.hc_ps_threshold(UMAX, 1 << 50) == (UMAX << 50) >> 32
    # no weight at all
    assert _select(hc, np.zeros(n, np.uint64), 9) == (-1, 0, 0)
    assert PS.select_ints(np.zeros(n, np.uint64), 9) == (-1, 0, 0)


def test_selection_word_is_the_third_stream(hc):
    from tests import philox_ref
    for seed, t, r in ((1, 0, 0), (0x5300714E ^ 5, 77, 2 ** 32 + 9), (2 ** 64 - 1, 2 ** 31 - 1, 2 ** 40)):
        w = philox_ref.philox4x32_10([t, 2, r & 0xFFFFFFFF, r >> 32], [seed & 0xFFFFFFFF, seed >> 32])
        assert hc.hc_ps_select_u(seed, t, r) == int(w[0])
        w1 = philox_ref.philox4x32_10([t, 1, r & 0xFFFFFFFF, r >> 32], [seed & 0xFFFFFFFF, seed >> 32])
        assert int(w1[0]) != int(w[0])


@pytest.mark.parametrize("model", [SU.AR, SU.LV, SU.FHN])
def test_pair_logw_matches_float64_density(hc, model):
    """pair_logw + the constant it drops against the float64 transition log-density, held to the bar of
    tests/test_gpu_simulate.py: 8 * max(e32, 2^-20 |lp|), e32 the largest error over the cases of the same formula
    in numpy float32."""
    rng = np.random.default_rng(5 + model)
    S, P, dt = SU.S_OF[model], SU.P_OF[model], SU.DT[model]
    step = {SU.AR: 3.0, SU.LV: 6.0, SU.FHN: 0.25}[model]
    rows = []
    for _ in range(300):
        true = np.asarray(SU.TRUE_THETA[model])
        th = (true + np.log(rng.uniform(0.9, 1.1, P)) if model == SU.LV else true * rng.uniform(0.9, 1.1, P))
        th = th.astype(np.float32)
        x = (np.asarray(SU.TRUE_X[model]) * rng.uniform(0.5, 1.5, S)).astype(np.float32)
        nxt = SU.step(model, x.astype(np.float64), th.astype(np.float64), dt, np.zeros(S))
        xt = (nxt + step * rng.uniform(-2.0, 2.0, S)).astype(np.float32)
        dropped = ctypes.c_float()
        th5 = np.zeros(5, np.float32)
        th5[:P] = th
        got = hc.hc_ps_pair_logw(model, x.ctypes.data, xt.ctypes.data, th5.ctypes.data, dt, ctypes.addressof(dropped))
        want = float(PS.trans_logp(model, x, xt, th, dt))
        lp32 = PS.trans_logp(model, x, xt, th, dt, np.float32)
        assert lp32.dtype == np.float32
        rows.append((float(got) + dropped.value, want, abs(float(lp32) - want)))
    got, want, e = (np.asarray(c) for c in zip(*rows))
    e32 = float(e.max())
    bar = 8.0 * np.maximum(e32, 2.0 ** -20 * np.abs(want))
    err = np.abs(got - want)
    print(f"model {model}: e32 {e32:.3e}, worst share of the bar {np.max(err / bar):.3f}")
    assert np.all(err <= bar), (model, float(np.max(err / bar)))
    # a dead particle: NaN, whatever the target
    dead = np.asarray([np.nan, 1.0] if model != SU.LV else [-1.0, 50.0], np.float32)[:S].copy()
    if model == SU.AR:
        dead = np.asarray([np.inf], np.float32)
    d = ctypes.c_float()
    th5 = np.zeros(5, np.float32)
    th5[:P] = np.asarray(SU.TRUE_THETA[model], np.float32)
    xt = np.asarray(SU.TRUE_X[model], np.float32)
    assert math.isnan(hc.hc_ps_pair_logw(model, dead.ctypes.data, xt.ctypes.data, th5.ctypes.data, dt,
                                         ctypes.addressof(d)))


def test_whole_draw_against_the_reference(hc):
    """ps::draw (prep, maximum, weights, selection, run serially) against ps_ref.backward_draw on the same particles:
    the weights within the q bar of tests/test_gpu_particle.py for logw errors of 2^-20 (1 + |logw|), the index the
    Python-int selection of the code's own weights; dead particles never; the terminal rule; a NaN target."""
    rng = np.random.default_rng(9)
    for model in (SU.AR, SU.LV, SU.FHN):
        S, P, dt, n = SU.S_OF[model], SU.P_OF[model], SU.DT[model], 128
        th = np.asarray(SU.TRUE_THETA[model], np.float32)
        th5 = np.zeros(5, np.float32)
        th5[:P] = th
        x = (np.asarray(SU.TRUE_X[model]) * rng.uniform(0.8, 1.2, (n, S))).astype(np.float32)
        x[3::8, 0] = np.nan
        if model == SU.LV:
            x[5::8, 1] = -0.5
        alive = SU.alive(model, x)
        xt = (np.asarray(SU.TRUE_X[model]) * rng.uniform(0.9, 1.1, S)).astype(np.float32)
        for U, target in ((0, xt), (0x9E3779B9, xt), (UMAX, xt), (12345, None)):
            q = np.zeros(n, np.uint64)
            m = ctypes.c_float()
            idx = hc.hc_ps_draw(model, x.ctypes.data, n, th5.ctypes.data, dt,
                                None if target is None else target.ctypes.data, U, q.ctypes.data,
                                ctypes.addressof(m))
            want_idx, W, _ = PS.select_ints(q, U)
            assert idx == want_idx and alive[idx] and not q[~alive].any() and int(q.max()) == ONE
            _, lw, m64, qref, _ = PS.backward_draw(model, x.astype(np.float64), None if target is None else
                                                   target[None].astype(np.float64), th.astype(np.float64), dt,
                                                   np.asarray([U], np.uint64), terminal=target is None)
            if target is None:
                assert np.array_equal(q, np.where(alive, ONE, 0).astype(np.uint64)) and m.value == 0.0
                continue
            lw, qr = lw[0], qref[0].astype(np.float64)
            d = 2.0 ** -20 * (1.0 + np.abs(lw[alive]).max())
            tol = qr * (math.expm1(2.0 * d) + (np.abs(np.where(alive, lw, 0.0) - m64[0]) + 2.0) * 2.0 ** -23) + 1.0
            assert np.all(np.abs(q.astype(np.float64) - qr) <= tol)
        bad = xt.copy()
        bad[0] = np.nan
        q = np.ones(n, np.uint64)
        m = ctypes.c_float()
        assert hc.hc_ps_draw(model, x.ctypes.data, n, th5.ctypes.data, dt, bad.ctypes.data, 7, q.ctypes.data,
                             ctypes.addressof(m)) == -1 and not q.any()


def test_abi_layout_of_the_descriptor():
    from viforssms_amd import _lib
    lib = ctypes.CDLL(HOSTCHECK)
    out = (ctypes.c_size_t * 2)()
    lib.vissm_host_abi_layout.restype = None
    lib.vissm_host_abi_layout(7, out)
    assert out[0] == ctypes.sizeof(_lib.PsDesc) == 28 and out[1] == _lib.PsDesc.dt.offset == 24
    assert [f[0] for f in _lib.PsDesc._fields_] == ["model", "K", "N", "M", "H", "t0", "dt"]


def test_library_refuses_without_gpu(hc):
    """Descriptor validation is host arithmetic that runs before any GPU call: with every pointer a dummy, a bad
    descriptor comes back VISSM_EINVAL; a good one with K = 0 is a no-op."""
    from viforssms_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    P = ctypes.addressof(buf)

    def call(desc, **null):
        names = ["theta", "cloud", "x_next", "paths", "x_first", "idx", "q_trace"]
        ptrs = [None if null.get(n) else P for n in names]
        return lib.vissm_particle_smooth(ctypes.byref(desc) if desc is not None else None, 1, 0, *ptrs, None)

    good = lambda **kw: _lib.PsDesc(**{**dict(model=_lib.MODEL_AR, K=0, N=128, M=64, H=4, t0=0, dt=1.0), **kw})
    assert call(good()) == 0
    assert call(good(), x_next=True, idx=True, q_trace=True) == 0                           # the optional ones
    assert call(good(model=_lib.MODEL_SV)) == -1 and b"SV" in lib.vissm_last_error()
    assert call(good(model=7)) == -1 and call(good(model=-1)) == -1 and call(None) == -1
    for n in (0, 32, 96, 2048, -64):
        assert call(good(N=n, M=64)) == -1, n
        assert b"particles" in lib.vissm_last_error()
    for m in (0, 1, 32, 63, 96, 256, -64):
        assert call(good(M=m)) == -1, m
        assert b"trajectories" in lib.vissm_last_error()
        assert hc.hc_ps_valid_m(m, 128) == 0
    assert call(good(M=128)) == 0 and hc.hc_ps_valid_m(128, 128) == 1 and hc.hc_ps_valid_m(64, 1024) == 1
    for kw in (dict(H=0), dict(H=-1), dict(K=-1), dict(K=65536), dict(t0=-1), dict(t0=2 ** 31 - 4, H=4)):
        assert call(good(**kw)) == -1, kw
    assert call(good(t0=2 ** 31 - 5, H=4)) == 0
    for name in ("theta", "cloud", "paths", "x_first"):
        assert call(good(), **{name: True}) == -1, name
        assert b"null pointer" in lib.vissm_last_error()
    # the LDS formula of DESIGN.md 4.9: 4 S N DEPTH + 4 L N + 4 (S + 1) 64 DEPTH + 768 NW + 256 (S + 1) with
    # DEPTH = clamp(16 KiB / (4 S N), 4, 32) and NW = min(4, N / 64) waves: two blocks per CU at the least
    lds = lib.vissm_particle_smooth_lds_bytes
    for model, S, L in ((_lib.MODEL_AR, 1, 1), (_lib.MODEL_LV, 2, 6), (_lib.MODEL_FHN, 2, 2)):
        for N in _lib.PF_PARTICLES:
            D, NW = min(32, max(4, 16384 // (4 * S * N))), min(4, N // 64)
            want = 4 * S * N * D + 4 * L * N + 4 * (S + 1) * 64 * D + 768 * NW + 256 * (S + 1)
            assert lds(model, N, 64) == want <= 160 * 1024 // 2
    assert lds(_lib.MODEL_LV, 1024, 1024) == 64256 and lds(_lib.MODEL_AR, 1024, 64) == 26112
    assert lds(_lib.MODEL_SV, 64, 64) == 0 and lds(_lib.MODEL_AR, 96, 64) == 0 and lds(_lib.MODEL_AR, 64, 128) == 0


def test_rts_against_dense_gaussian():
    """The RTS means and variances against the posterior of the joint Gaussian of (x_1 .. x_T) given the observed
    entries, written out densely."""
    rng = np.random.default_rng(8)
    th, x0, T, r = [0.3, 0.8, math.log(0.7)], 1.5, 12, 0.5
    b = (rng.uniform(size=T) < 0.6).astype(float)
    b[0], b[-1] = 1.0, 0.0
    y = rng.normal(1.5, 1.0, T)
    phi, s2 = th[1], math.exp(2 * th[2])
    mean, rows, m, A = np.zeros(T), [], x0, np.zeros(T)
    for t in range(T):
        m = phi * m + th[0]
        A = phi * A
        A[t] = 1.0
        mean[t] = m
        rows.append(A.copy())
    R = np.stack(rows)
    cov = s2 * R @ R.T                               # prior covariance of the states
    idx = np.where(b > 0)[0]
    Sy = cov[np.ix_(idx, idx)] + r * r * np.eye(idx.size)
    G = cov[:, idx] @ np.linalg.inv(Sy)
    want_m = mean + G @ (y[idx] - mean[idx])
    want_v = np.diag(cov - G @ cov[idx, :])
    got = PS.rts_ar(th, x0, y, b, r)
    assert np.allclose(got["ms"], want_m, rtol=0, atol=1e-10) and np.allclose(got["vs"], want_v, rtol=0, atol=1e-10)
    assert np.all(got["vs"] <= got["vf"] + 1e-12) and got["vs"][-1] == got["vf"][-1]


def test_reference_meets_its_own_bars():
    """Two independent seeds of the numpy smoother against each other and against RTS at the GPU test's shape
    (K = 256, N = 256, M = 64): the bars the kernel is held to are ones a correct smoother of this construction
    meets, and the filter's own means miss (b)."""
    rts = PS.stat_rts()
    a, b = PS.reference_paths(101), PS.reference_paths(202)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    ma, mb = PS.stat_moments(a), PS.stat_moments(b)
    for (mean, se, sd), (mean_r, se_r, _) in ((ma, mb), (mb, ma)):
        bars = PS.stat_bars(mean, se, sd, mean_r, se_r, rts)
        print(bars)
        assert all(v[0] for v in bars.values()), bars
    s = np.sqrt(rts["vs"])
    gap = np.abs(rts["mf"] - rts["ms"]) / s
    print(f"filtering mean against smoothing mean: up to {gap.max():.3f} sd; sd ratio down to "
          f"{np.sqrt(rts['vs'] / rts['vf']).min():.3f}")
    assert gap.max() > 4.0 * PS.MEAN_BAR                  # the bars discriminate: the filter's bands miss (b)
