"""The correlated pseudo-marginal chain of the stochastic-volatility model without a GPU: cpm_math.hpp as the host build
compiles it (libvissm_hostcheck.so: the code the kernels run) against numpy and math.erfc (tests/cpm_ref.py); the
refusals of the two C entries, of the wrappers and of the product path, which are host arithmetic; the command-line
option; and the numpy reference itself -- the sorted filter's ratio noise on two seeds against each other, and the
reference chain against the exact (grid) posterior of the T = 64 fixture."""
import ctypes
import math
import os
import types

import numpy as np
import pytest

from tests import cpm_ref as CR
from tests import pmmh_ref as MR
from tests import svf_ref as SR
from tests import svpmmh_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK = os.path.join(ROOT, "viforssms_amd", "libvissm_hostcheck.so")
INF = float("inf")


@pytest.fixture(scope="module")
def hc():
    lib = ctypes.CDLL(HOSTCHECK)
    f, u32, i = ctypes.c_float, ctypes.c_uint32, ctypes.c_int
    for name, res, args in (("hc_cpm_cn", f, [f] * 4), ("hc_cpm_sigma", f, [f]), ("hc_cpm_valid_rho", i, [f]),
                            ("hc_cpm_sort_key", u32, [f]), ("hc_cpm_key_value", f, [u32]),
                            ("hc_cpm_resample_u", u32, [f])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


SPECIAL = np.array([0.0, -0.0, 1.0, -1.0, 1e-45, -1e-45, 1.1754944e-38, 3.4028235e38, -3.4028235e38, 0.1, 1 / 3, 8.5,
                    -8.5, 1e-20, 1e20], np.float32)


def test_cn_is_numpy_float32_bit_for_bit(hc):
    """fl32(fl32(rho u) + fl32(sigma eps)) over random and special inputs, for the rho the product path allows; sigma
    is float32(sqrt(1 - rho^2)) with the root in float64."""
    rng = np.random.default_rng(0)
    for rho in (0.0, 0.5, 0.9, 0.99, 0.999, 0.9999, 1 / 3):
        rho32 = np.float32(rho)
        sig = CR.sigma_of(rho32)
        assert _bits(hc.hc_cpm_sigma(rho32)) == _bits(sig)
        u = np.concatenate([rng.standard_normal(2000).astype(np.float32), np.repeat(SPECIAL, len(SPECIAL))])
        e = np.concatenate([rng.standard_normal(2000).astype(np.float32), np.tile(SPECIAL, len(SPECIAL))])
        with np.errstate(over="ignore", invalid="ignore"):
            want = CR.cn(u, e, rho32)
        got = np.array([hc.hc_cpm_cn(float(a), float(b), float(rho32), float(sig)) for a, b in zip(u, e)], np.float32)
        both_nan = np.isnan(want) & np.isnan(got)
        assert np.array_equal(_bits(got)[~both_nan], _bits(want)[~both_nan]), rho
    for rho, ok in ((0.0, 1), (0.9999, 1), (np.nextafter(np.float32(1), np.float32(0)), 1), (1.0, 0), (-1e-9, 0),
                    (float("nan"), 0), (INF, 0), (2.0, 0)):
        assert hc.hc_cpm_valid_rho(float(rho)) == ok, rho


def test_sort_key_orders_as_numpy_and_key_value_inverts_it(hc):
    """On a vector mixing negatives, positives, +-0, duplicates, +-inf and NaN the unsigned order of the keys is
    np.sort's order of the vector with everything not finite made NaN first (the filter's death rule: a particle that
    is not finite is the quiet NaN and sorts last), -0 comes before +0, and key_value gives the bits back."""
    rng = np.random.default_rng(1)
    v = np.concatenate([rng.standard_normal(200) * 10.0 ** rng.integers(-30, 30, 200), SPECIAL, SPECIAL,
                        [np.inf, -np.inf, np.nan, -np.nan, np.inf]]).astype(np.float32)
    rng.shuffle(v)
    keys = np.array([hc.hc_cpm_sort_key(float(x)) for x in v], np.uint32)
    assert np.array_equal(keys, CR.sort_key(v))                      # the numpy restatement
    finite = np.isfinite(v)
    assert np.all(keys[~finite] == 0xFFFFFFFF) and np.all(keys[finite] != 0xFFFFFFFF)
    back = np.array([hc.hc_cpm_key_value(int(k)) for k in keys], np.float32)
    assert np.array_equal(_bits(back[finite]), _bits(v[finite])) and np.isnan(back[~finite]).all()
    by_key = back[np.argsort(keys, kind="stable")]
    want = np.sort(np.where(finite, v, np.float32(np.nan)))
    assert np.array_equal(by_key, want, equal_nan=True)
    zeros = by_key[by_key == 0.0]
    assert len(zeros) == 4 and np.signbit(zeros).tolist() == [True, True, False, False]
    assert np.array_equal(_bits(CR.sort_states(v)), _bits(by_key))


def test_resample_u_against_math_erfc(hc):
    """Within one unit of floor(erfc(-x / sqrt 2) / 2 * 2^24) from math.erfc at +-8, 0 and 10^4 random points; clamped
    to [0, 2^24 - 1] at both ends."""
    rng = np.random.default_rng(2)
    xs = np.concatenate([[8.0, -8.0, 0.0, -0.0], rng.standard_normal(10000) * 2.0]).astype(np.float32)
    want = CR.resample_u(xs)
    got = np.array([hc.hc_cpm_resample_u(float(x)) for x in xs], np.int64)
    assert np.abs(got - want).max() <= 1
    assert got[2] == got[3] == 1 << 23 and got[0] == (1 << 24) - 1 and got[1] == 0
    for x, u in ((40.0, (1 << 24) - 1), (INF, (1 << 24) - 1), (5.5, (1 << 24) - 1), (-40.0, 0), (-INF, 0), (-6.0, 0)):
        assert hc.hc_cpm_resample_u(x) == u, x
    assert want.min() >= 0 and want.max() <= (1 << 24) - 1


# ----------------------------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------------------------
def test_abi():
    from viforssms_amd import _lib
    assert len(_lib.SIGNATURES["vissm_sv_filter_sorted"][1]) == 1 + 12 + 1
    assert len(_lib.SIGNATURES["vissm_sv_cpmmh"][1]) == 3 + 6 + 4 + 3 + 13 + 1
    assert _lib.SIGNATURES["vissm_sv_cpmmh"][1][12] is ctypes.c_float


def test_filter_entry_refuses_without_gpu():
    from viforssms_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    A = ctypes.addressof(buf)
    names = ["theta", "x_start", "obs", "aux_n", "aux_r", "loglik", "ll_inc", "cloud", "sorted_trace", "q_trace",
             "anc_trace", "u_trace"]

    def call(desc, **ptr):
        ptrs = [ptr.get(n, A) for n in names]
        return lib.vissm_sv_filter_sorted(ctypes.byref(desc) if desc is not None else None, *ptrs, None)

    one = lambda **kw: _lib.PfDesc(**{**dict(model=_lib.MODEL_SV, K=1, N=64, H=4, t0=0, T_total=4, dt=1.0,
                                             obs_std=0.0), **kw})
    assert call(None) == -1 and b"null descriptor" in lib.vissm_last_error()
    for model in (_lib.MODEL_AR, _lib.MODEL_LV, _lib.MODEL_FHN, 7, -1):
        assert call(one(model=model)) == -1 and b"SV" in lib.vissm_last_error()
    for n in (0, 1, 32, 63, 96, 2048, -64):
        assert call(one(N=n)) == -1 and b"particles" in lib.vissm_last_error(), n
    for kw in (dict(K=-1), dict(H=-1, T_total=-1), dict(K=2 ** 25)):
        assert call(one(**kw)) == -1, kw
    # no chaining in time: t0 = 0 and H = T_total only
    for kw in (dict(t0=1, H=3), dict(H=3), dict(H=5), dict(t0=1)):
        assert call(one(**kw)) == -1 and b"whole series" in lib.vissm_last_error(), kw
    for dt in (0.0, -1.0, float("nan"), INF):
        assert call(one(dt=dt)) == -1 and b"dt" in lib.vissm_last_error(), dt
    for name in names[:7]:
        assert call(one(), **{name: None}) == -1 and b"null pointer" in lib.vissm_last_error(), name
    assert call(one(), aux_n=A + 4) == -1 and b"aligned" in lib.vissm_last_error()
    assert call(one(K=0)) == 0                                       # nothing to do, before any GPU call
    for n in _lib.PF_PARTICLES:
        want = 8 * n + 4 * n + 192 + (8 * n if n > 64 else 4)
        assert lib.vissm_sv_filter_sorted_lds_bytes(n) == want
        assert lib.vissm_sv_cpmmh_lds_bytes(n) == want + 4 * n + 256
    for n in (0, 1, 63, 96, 2048, -64):
        assert lib.vissm_sv_filter_sorted_lds_bytes(n) == 0 and lib.vissm_sv_cpmmh_lds_bytes(n) == 0


def test_chain_entry_refuses_without_gpu():
    """Everything vissm_sv_pmmh_adaptive refuses, rho outside [0, 1) or NaN, a null or misaligned aux pointer."""
    from viforssms_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    A = ctypes.addressof(buf)
    head = ["theta_cur", "ll_cur", "chol_in", "prior", "h_start", "obs"]
    aux = ["aux_n", "aux_r", "aux_sel"]
    tail = ["theta_chain", "ll_chain", "accept", "theta_end", "ll_end", "chol_end", "theta_prop", "ll_prop", "logu",
            "xi_trace", "alpha_trace", "eta_trace", "chol_trace"]

    def call(desc, adapt_end=0, target=0.234, gamma=0.5, rho=0.99, **ptr):
        p = lambda names: [ptr.get(n, A) for n in names]
        return lib.vissm_sv_cpmmh(ctypes.byref(desc) if desc is not None else None, 1, 0, *p(head), adapt_end, target,
                                  gamma, rho, *p(aux), *p(tail), None)

    one = lambda **kw: _lib.PmmhDesc(**{**dict(model=_lib.MODEL_SV, C=1, N=64, n_iter=1, it0=0, T_total=4, dt=1.0,
                                               obs_std=0.0), **kw})
    assert call(None) == -1 and b"null descriptor" in lib.vissm_last_error()
    for model in (_lib.MODEL_AR, _lib.MODEL_LV, _lib.MODEL_FHN, 7, -1):
        assert call(one(model=model)) == -1 and b"SV" in lib.vissm_last_error()
    for n in (0, 1, 32, 63, 96, 2048, -64):
        assert call(one(N=n)) == -1 and b"particles" in lib.vissm_last_error(), n
    for c in (0, -1):
        assert call(one(C=c)) == -1 and b"chains" in lib.vissm_last_error()
    for kw in (dict(n_iter=-1), dict(it0=-1), dict(it0=2 ** 31 - 1, n_iter=1)):
        assert call(one(**kw)) == -1 and b"iterations" in lib.vissm_last_error(), kw
    for t in (-1, 2 ** 31 - 1):
        assert call(one(T_total=t)) == -1 and b"T_total" in lib.vissm_last_error(), t
    for dt in (0.0, -1.0, float("nan"), INF):
        assert call(one(dt=dt)) == -1 and b"dt" in lib.vissm_last_error(), dt
    assert call(one(), adapt_end=-1) == -1 and b"adapt_end" in lib.vissm_last_error()
    for t in (0.0, 1.0, float("nan")):
        assert call(one(), target=t) == -1 and b"target_accept" in lib.vissm_last_error()
    for g in (0.0, 1.5, float("nan")):
        assert call(one(), gamma=g) == -1 and b"gamma" in lib.vissm_last_error()
    for rho in (1.0, -0.01, 2.0, float("nan"), INF, -INF):
        assert call(one(), rho=rho) == -1 and b"rho" in lib.vissm_last_error(), rho
    for name in head + tail[:6]:
        assert call(one(), **{name: None}) == -1 and b"null pointer" in lib.vissm_last_error(), name
    for name in aux:
        assert call(one(), **{name: None}) == -1 and b"aux" in lib.vissm_last_error(), name
    assert call(one(), aux_n=A + 8) == -1 and b"aligned" in lib.vissm_last_error()


def test_python_refusals_without_gpu():
    import torch
    from viforssms_amd import _lib, ops
    th, ll = torch.zeros(2, 4), torch.zeros(2, dtype=torch.float64)
    L, pr, h0, y = torch.eye(4).repeat(2, 1, 1), torch.ones(4, 2), torch.zeros(1), torch.ones(9)
    an, ar, sel = torch.zeros(2, 2, 2, 64, 4), torch.zeros(2, 2, 8), torch.zeros(2, dtype=torch.int32)

    def run(N=64, dt=1.0, rho=0.99, n_iter=1, it0=0, row0=0, **kw):
        return ops.sv_cpmmh(th, ll, L, pr, h0, y, dt, N, n_iter, 1, row0, rho, an, ar, sel, it0=it0, **kw)

    for n in (0, 32, 96, 2048):
        with pytest.raises(ValueError, match="particles"):
            run(N=n)
    for dt in (0.0, -1.0, float("nan"), INF):
        with pytest.raises(ValueError, match="dt"):
            run(dt=dt)
    for rho in (1.0, -0.1, float("nan"), 1.0 - 1e-9):               # the last rounds to 1 in fp32
        with pytest.raises(ValueError, match="rho"):
            run(rho=rho)
    for kw in (dict(n_iter=-1), dict(it0=-1), dict(it0=2 ** 31 - 1)):
        with pytest.raises(ValueError, match="iterations"):
            run(**kw)
    for kw, msg in ((dict(adapt_end=-1), "adapt_end"), (dict(target_accept=1.0), "target_accept"),
                    (dict(gamma=0.0), "gamma")):
        with pytest.raises(ValueError, match=msg):
            run(**kw)
    with pytest.raises(ValueError, match="row0"):
        run(row0=-1)
    with pytest.raises(_lib.VissmError, match="GPU only"):
        run()
    for kw in (dict(N=96), dict(dt=0.0)):
        with pytest.raises(ValueError):
            ops.sv_filter_sorted(th, h0, y, **{**dict(dt=1.0, N=64), **kw}, aux_n=an[:, 0], aux_r=ar[:, 0])
    with pytest.raises(_lib.VissmError, match="GPU only"):
        ops.sv_filter_sorted(th, h0, y, 1.0, 64, an[:, 0].contiguous(), ar[:, 0].contiguous())
    for kw in (dict(C=0), dict(T=0), dict(N=96), dict(row0=-1)):
        with pytest.raises(ValueError, match="cpm_fresh_aux"):
            ops.cpm_fresh_aux(**{**dict(C=2, T=8, N=64, seed=1, row0=0), **kw})
    assert ops.cpm_groups(1) == 1 and ops.cpm_groups(4) == 1 and ops.cpm_groups(5) == 2 and ops.cpm_groups(1508) == 377


def test_product_refusals_without_gpu():
    """volatility_mcmc refuses a correlation outside [0, 0.9999], theta_mcmc any but 0, before touching the device."""
    from viforssms_amd import _lib
    from viforssms_amd.diagnostics import PosteriorDiagnostics

    class Stub(PosteriorDiagnostics):
        def __init__(self, model_id, family, obs):
            self.mdef = types.SimpleNamespace(model_id=model_id, family=family)
            self.p_local, self.obs, self.filter_data = 8, obs, None

        def target_len(self):
            return len(self.obs) - 1

    y = np.linspace(1.0, 2.0, 21)
    sv = Stub(_lib.MODEL_SV, "sv", y)
    for rho in (-0.1, 1.0, 0.99995, float("nan"), INF):
        with pytest.raises(ValueError, match="correlation"):
            sv.volatility_mcmc(4, 64, 10, 2, correlation=rho)
    for family, model_id in (("ar", _lib.MODEL_AR), ("lv", _lib.MODEL_LV), ("fhn", _lib.MODEL_FHN)):
        with pytest.raises(ValueError, match="correlation"):
            Stub(model_id, family, y).theta_mcmc(4, 64, 10, 2, correlation=0.99)
    with pytest.raises(ValueError, match="n_particles"):            # the other refusals are unchanged
        sv.volatility_mcmc(4, 96, 10, 2, correlation=0.99)


def test_cli_option():
    from viforssms_amd import sv
    for bad in (["--mcmc-corr", "0.99"], ["--mcmc", "8", "64", "100", "m.npz", "--mcmc-corr", "1.0"],
                ["--mcmc", "8", "64", "100", "m.npz", "--mcmc-corr", "-0.5"],
                ["--mcmc", "8", "64", "100", "m.npz", "--mcmc-corr", "high"]):
        with pytest.raises(SystemExit):
            sv.run(bad)


# ----------------------------------------------------------------------------------------------------------------
# the numpy reference
# ----------------------------------------------------------------------------------------------------------------
def test_reference_ratio_noise_on_two_seeds():
    """sd(ll(aux') - ll(aux)) of the reference's sorted filter (T = 256, N = 64, K = 256): the two seeds agree within
    the project's sd bar [0.8, 1.25] at rho = 0.99 and at rho = 0 (with 256 draws 4 se of a ratio of two sds is about
    25 %), the correlated noise is several times below the independent one, and without the sort it is not."""
    s = {(rho, seed): CR.reference_ratio_noise(ROOT, rho, seed) for rho in (0.99, 0.0) for seed in (1, 2)}
    print(s)
    for rho in (0.99, 0.0):
        assert 0.8 <= s[rho, 1] / s[rho, 2] <= 1.25, rho
    assert s[0.99, 1] / s[0.0, 1] <= 0.25 and s[0.99, 2] / s[0.0, 2] <= 0.25
    y = CR.noise_series(ROOT).astype(np.float64)
    th = np.tile(np.asarray(SR.PARAM_INIT), (CR.NOISE_K, 1))
    unsorted = CR.ratio_noise(lambda un, ur: CR.run_sorted_filter(th, CR.NOISE_H0, y, CR.NOISE_DT, CR.NOISE_N,
                                                                  un.astype(np.float64), ur.astype(np.float64),
                                                                  sort=False), 0.99, 1)
    print("unsorted", unsorted)
    assert unsorted >= 2.0 * s[0.99, 1]


@pytest.mark.parametrize("seed", [11, 12])
def test_reference_chain_meets_the_exact_posterior(seed):
    """The reference chain on the T = 64 fixture, C = 64, N = 64, rho = 0.99, the fixture's L and a spread start:
    pmmh_ref.stat_bars against truth("exact") -- the exact chain's acceptance included, which the ordinary PMMH
    reference at N = 64 misses by 12 se.  300 iterations of which 100 are dropped: the shortest of 700/200, 500/150,
    400/120 and 300/100 tried, all of which held for both seeds (about 10 s each)."""
    t = VR.truth("exact")
    r = CR.cpm_chain(VR.stat_start(t, 64, seed), t["L"], t["prior"], SR.FIX_H0, VR.stat_series(), 1.0, 64, 300, 0.99,
                     np.random.default_rng(seed))
    s = MR.summarise(r["theta"][:, 100:], r["accept"][:, 100:])
    bars = MR.stat_bars(s, t)
    print({k: np.round(v, 4) for k, v in s.items()}, bars)
    assert bars["ok"], bars
