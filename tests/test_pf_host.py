"""The particle filter without a GPU: the integer half of csrc/pf_math.hpp (the code the kernel runs, built for the
host in libvissm_hostcheck.so) against Python big-int arithmetic; the library's refusals, which are host arithmetic;
and the statistical bars of tests/test_gpu_particle.py for the numpy reference alone (tests/pf_ref.py), two seeds
against each other and against the exact Kalman log-likelihood."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import pf_ref as PR
from tests import sim_util as SU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK = os.path.join(ROOT, "viforssms_amd", "libvissm_hostcheck.so")
UMAX = (1 << 24) - 1
ONE = 1 << 40


@pytest.fixture(scope="module")
def hc():
    lib = ctypes.CDLL(HOSTCHECK)
    lib.hc_pf_quantise.restype = ctypes.c_uint64
    lib.hc_pf_quantise.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_int]
    lib.hc_pf_threshold.restype = ctypes.c_uint64
    lib.hc_pf_threshold.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int]
    lib.hc_pf_resample.restype = ctypes.c_uint64
    lib.hc_pf_resample.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    lib.hc_pf_resample_u.restype = ctypes.c_uint32
    lib.hc_pf_resample_u.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64]
    lib.hc_pf_logw.restype = ctypes.c_float
    lib.hc_pf_logw.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_float]
    lib.hc_pf_ll_increment.restype = ctypes.c_double
    lib.hc_pf_ll_increment.argtypes = [ctypes.c_float, ctypes.c_uint64, ctypes.c_int]
    return lib


def _resample(hc, q, U):
    q = np.ascontiguousarray(q, np.uint64)
    n = q.size
    anc, C = np.full(n, -7, np.int32), np.zeros(n, np.uint64)
    W = hc.hc_pf_resample(q.ctypes.data, n, U, anc.ctypes.data, C.ctypes.data)
    return anc, C, W


def _weight_cases(n, rng):
    """Edge weights: a single survivor (W = 2^40); every weight 2^40 (W = N 2^40, 2^50 at N = 1024: with U = 0 every
    threshold j 2^40 falls exactly on C_{j-1}); one below it; runs of zeros; three unit weights behind N - 3 zeros;
    weights spread over thirty e-folds."""
    one = np.zeros(n, np.uint64)
    one[n // 3] = ONE
    full = np.full(n, ONE, np.uint64)
    below = full.copy()
    below[-1] -= np.uint64(1)
    runs = rng.integers(0, ONE, n, dtype=np.uint64)
    runs[(np.arange(n) // 7) % 2 == 1] = 0
    runs[5] = ONE
    tail = np.zeros(n, np.uint64)
    tail[-3:] = 1
    spread = np.floor(np.exp(rng.uniform(-30.0, 0.0, n)) * ONE).astype(np.uint64)
    spread[0] = ONE
    return {"survivor": one, "full": full, "below": below, "runs": runs, "tail": tail, "spread": spread}


@pytest.mark.parametrize("n", [64, 1024])
def test_resampling_matches_python_ints(hc, n):
    rng = np.random.default_rng(n)
    log2n = n.bit_length() - 1
    for name, q in _weight_cases(n, rng).items():
        for U in (0, 1, UMAX // 2, UMAX):
            want, W = PR.systematic_ints(q, U)
            anc, C, Wc = _resample(hc, q, U)
            assert Wc == W and [int(c) for c in C] == list(np.cumsum([int(v) for v in q], dtype=object)), name
            assert anc.tolist() == want, (name, U)
            assert max(want) <= n - 1 and all(int(q[a]) > 0 for a in want), (name, U)
            for j in (0, 1, n // 2, n - 1):
                tau = (((j << 24) + U) * W) >> (24 + log2n)
                assert hc.hc_pf_threshold(j, U, W, log2n) == tau and tau < W
            v_anc, v_W = PR.systematic_u64(q[None, :], np.asarray([U], np.uint64))   # the reference's vectorised form
            assert v_anc[0].tolist() == want and int(v_W[0]) == W, (name, U)
    # W near 2^50: the largest sum N = 1024 can reach, thresholds at the last slot
    W = 1024 * ONE
    assert hc.hc_pf_threshold(1023, UMAX, W, 10) == (((1023 << 24) + UMAX) * W) >> 34
    # tau exactly on a C_i: the particle whose cumulative sum equals tau is passed over (C_i <= tau counts it)
    q = np.full(n, ONE, np.uint64)
    anc, _, _ = _resample(hc, q, 0)
    assert anc.tolist() == list(range(n))
    # no weight at all: W = 0 and the ancestors are left alone
    anc, _, W0 = _resample(hc, np.zeros(n, np.uint64), 9)
    assert W0 == 0 and (anc == -7).all()


def test_quantise_matches_fp32_exp(hc):
    rng = np.random.default_rng(3)
    m = np.float32(-7.25)
    lw = np.concatenate([[m, m - np.float32(100.0), np.float32(-np.inf)],
                         (m - rng.uniform(0.0, 30.0, 500)).astype(np.float32)]).astype(np.float32)
    for v in lw:
        got = hc.hc_pf_quantise(float(v), float(m), 1)
        e = np.exp(np.float32(v - m), dtype=np.float32)
        want = int(np.float32(e) * np.float32(2.0 ** 40))
        # libm's float exp and numpy's agree to an ulp: 2^-23 relative, and one unit for the truncation
        assert abs(got - want) <= want * 2.0 ** -22 + 1, (v, got, want)
        assert hc.hc_pf_quantise(float(v), float(m), 0) == 0
    assert hc.hc_pf_quantise(float(m), float(m), 1) == ONE
    assert hc.hc_pf_quantise(-np.inf, -np.inf, 1) == 0
    # the reference's quantise is the same rule
    mm, q = PR.quantise(lw.astype(np.float64), np.ones(lw.size, bool))
    assert mm == float(m) and int(q[0]) == ONE and int(q[2]) == 0


def test_logw_increment_and_u(hc):
    from tests import philox_ref
    rng = np.random.default_rng(4)
    for model in (SU.AR, SU.LV, SU.FHN):
        S = SU.S_OF[model]
        for b in ([[1.0], [0.5]] if S == 1 else [[1.0, 1.0], [0.0, 1.0], [1.0, 0.0]]):
            x = rng.normal(3.0, 2.0, S).astype(np.float32)
            y = np.where(np.asarray(b) > 0, rng.normal(3.0, 2.0, S), np.nan).astype(np.float32)   # unobserved: filler
            bb = np.asarray(b, np.float32)
            got = hc.hc_pf_logw(model, x.ctypes.data, y.ctypes.data, bb.ctypes.data, 0.7)
            want = float(PR.obs_logw(x.astype(np.float64)[None], y, bb, np.float32(0.7))[0])
            assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (model, b)
    assert abs(hc.hc_pf_ll_increment(-2.5, 3 * ONE + 17, 256) - PR.ll_increment(-2.5, 3 * ONE + 17, 256)) < 1e-12
    for seed, t, r in ((1, 0, 0), (0xF117E2ED ^ 5, 77, 2 ** 32 + 9), (2 ** 64 - 1, 2 ** 31 - 1, 2 ** 40)):
        w = philox_ref.philox4x32_10([t, 1, r & 0xFFFFFFFF, r >> 32], [seed & 0xFFFFFFFF, seed >> 32])
        assert hc.hc_pf_resample_u(seed, t, r) == int(w[0]) >> 8


def test_abi_layout_of_the_descriptor():
    from viforssms_amd import _lib
    lib = ctypes.CDLL(HOSTCHECK)
    out = (ctypes.c_size_t * 2)()
    lib.vissm_host_abi_layout.restype = None
    lib.vissm_host_abi_layout(6, out)
    assert out[0] == ctypes.sizeof(_lib.PfDesc) and out[1] == _lib.PfDesc.obs_std.offset
    assert [f[0] for f in _lib.PfDesc._fields_] == ["model", "K", "N", "H", "t0", "T_total", "dt", "obs_std"]


def test_library_refuses_without_gpu():
    """Descriptor validation is host arithmetic that runs before any GPU call: with every pointer a dummy, a bad
    descriptor comes back VISSM_EINVAL; a good one with K = 0 is a no-op."""
    from viforssms_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    P = ctypes.addressof(buf)

    def call(desc, **null):
        names = ["theta", "x_start", "obs", "obs_bin", "loglik_in", "loglik", "ll_inc", "ess", "state_end", "cloud",
                 "q_trace", "anc_trace"]
        ptrs = [None if null.get(n) else P for n in names]
        return lib.vissm_particle_filter(ctypes.byref(desc) if desc is not None else None, 1, 0, *ptrs, None)

    good = lambda **kw: _lib.PfDesc(**{**dict(model=_lib.MODEL_AR, K=0, N=64, H=4, t0=0, T_total=4, dt=1.0,
                                              obs_std=1.0), **kw})
    assert call(good()) == 0
    assert call(good(), loglik_in=True, cloud=True, q_trace=True, anc_trace=True) == 0      # the optional ones
    assert lib.vissm_particle_filter_lds_bytes(_lib.MODEL_LV, 1024) == 4 * 2 * 1024 * 16 + 8 * 1024 + 8 * 1024 + 128 + 320
    assert lib.vissm_particle_filter_lds_bytes(_lib.MODEL_AR, 64) == 4 * 64 * 64 + 8 * 64 + 4 * 64 + 512 + 320
    assert lib.vissm_particle_filter_lds_bytes(_lib.MODEL_SV, 64) == 0
    assert lib.vissm_particle_filter_lds_bytes(_lib.MODEL_AR, 96) == 0
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
    assert call(good(t0=2, H=3, T_total=4)) == -1                                           # past the observations
    big = 2 ** 31 - 1
    assert call(good(model=_lib.MODEL_LV, t0=2 ** 30, H=8, T_total=big)) == -1              # (t0 + H) S reaches 2^31
    assert b"2^31" in lib.vissm_last_error()
    assert call(good(model=_lib.MODEL_LV, t0=2 ** 30 - 8, H=7, T_total=big)) == 0           # one below it, K = 0
    assert call(good(t0=big - 3, H=3, T_total=big)) == 0
    assert call(good(t0=big, H=big, T_total=big)) == -1
    assert call(good(K=2 ** 22, N=1024)) == -1                                              # K N reaches 2^31


# ----------------------------------------------------------------------------------------------------------------
# the statistical bars, for the reference alone
# ----------------------------------------------------------------------------------------------------------------
def test_fixture_is_the_documented_series():
    obs, obs_bin = PR.stat_case()
    y, b = PR.ar_dataset(T=64, frac=0.7, obs_std=1.0, seed=int(np.load(PR.FIXTURE)["seed"]))
    assert obs.shape == (1, 64) and obs.dtype == np.float32 and np.array_equal(obs_bin, b)
    assert np.allclose(obs, y, rtol=0, atol=1e-5)
    assert 0.6 <= obs_bin.mean() <= 0.8


def test_reference_meets_its_own_bars():
    """Two independent seeds of the numpy filter against each other and against Kalman: the bars the kernel is held
    to are ones a correct filter of this construction meets (K = 256 against K_r = 1024, and the two swapped)."""
    obs, obs_bin = PR.stat_case()
    L = PR.kalman_ar_loglik(SU.TRUE_THETA[SU.AR], SU.TRUE_X[SU.AR][0], obs[0], obs_bin[0], 1.0)
    a, b = PR.reference_logliks(101), PR.reference_logliks(202)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    for small, large in ((a[:256], b), (b[:256], a)):
        mu, s, mu_r, s_r = small.mean(), small.std(ddof=1), large.mean(), large.std(ddof=1)
        bars = PR.stat_bars(mu, s, small.size, mu_r, s_r, large.size, L)
        print(f"L {L:.4f} mu {mu:.4f} s {s:.4f} mu_r {mu_r:.4f} s_r {s_r:.4f} L - mu_r {L - mu_r:.4f} {bars}")
        assert all(bars.values()), bars
        assert 0.0 < L - mu_r < s_r * s_r          # Jensen: below Kalman by about s^2 / 2


def test_kalman_against_dense_gaussian():
    """The Kalman recursion against the joint Gaussian of the observed entries written out densely."""
    rng = np.random.default_rng(8)
    th, x0, T, r = [0.3, 0.8, math.log(0.7)], 1.5, 12, 0.5
    b = (rng.uniform(size=T) < 0.6).astype(float)
    b[0] = 1.0
    y = rng.normal(1.5, 1.0, T)
    phi, s2 = th[1], math.exp(2 * th[2])
    mean = np.zeros(T)
    cov = np.zeros((T, T))
    m, A = x0, np.zeros(T)          # x_t = m_t + sum_j A_tj n_j
    rows = []
    for t in range(T):
        m = phi * m + th[0]
        A = phi * A
        A[t] = 1.0
        mean[t] = m
        rows.append(A.copy())
    R = np.stack(rows)
    cov = s2 * R @ R.T + r * r * np.eye(T)
    idx = np.where(b > 0)[0]
    d = y[idx] - mean[idx]
    Sg = cov[np.ix_(idx, idx)]
    want = -0.5 * (d @ np.linalg.solve(Sg, d) + np.linalg.slogdet(2 * np.pi * Sg)[1])
    assert abs(PR.kalman_ar_loglik(th, x0, y, b, r) - want) < 1e-9
