"""The adaptive chains without a GPU: mh::adapt, mh::accept_prob and mh::adapt_eta (csrc/mh_math.hpp, the code the
kernel's thread 0 runs, built for the host in libvissm_hostcheck.so) against the numpy restatement of
tests/pmmh_adapt_ref.py; the library's, ops' and the product's refusals, which are host arithmetic; the ABI; the
command-line option; and the statistical conditions of tests/test_gpu_pmmh_adapt.py for the numpy reference alone."""
import ctypes
import math
import os
import types

import numpy as np
import pytest

from tests import pf_ref as PR
from tests import pmmh_adapt_ref as AR
from tests import pmmh_ref as MR
from tests import sim_util as SU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK = os.path.join(ROOT, "viforssms_amd", "libvissm_hostcheck.so")
FP = ctypes.POINTER(ctypes.c_float)
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def hc():
    lib = ctypes.CDLL(HOSTCHECK)
    d, i = ctypes.c_double, ctypes.c_int
    lib.hc_mh_alpha.restype, lib.hc_mh_alpha.argtypes = d, [d] * 4
    lib.hc_mh_eta.restype, lib.hc_mh_eta.argtypes = d, [i, ctypes.c_int64, d]
    lib.hc_mh_adapt.restype, lib.hc_mh_adapt.argtypes = i, [FP, FP, d, d, d, i]
    return lib


def _adapt(hc, L, xi, al, et, target):
    """(L' [P, P] fp32 with the upper part as it came in, changed) from the host build of mh::adapt."""
    out = np.ascontiguousarray(L, np.float32).copy()
    z = np.ascontiguousarray(xi, np.float32)
    rc = hc.hc_mh_adapt(out.ctypes.data_as(FP), z.ctypes.data_as(FP), al, et, target, L.shape[0])
    assert rc in (0, 1)
    return out, bool(rc)


def _factor(rng, P, scale=1.0):
    L = np.tril(rng.normal(0, 0.3, (P, P)))
    L[np.diag_indices(P)] = rng.uniform(0.2, 1.5, P)
    L[0] *= scale
    return L.astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------
# the update
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [3, 4, 5])
def test_update_bitwise_identity_and_invariants(hc, P):
    """Over 300 random cases per P -- both signs of d, eta = 1 and a small eta, factors whose first row is up to 100
    times the others -- the host build of mh::adapt equals the numpy restatement bit for bit; L' L'^T equals
    L (I + d xi xi^T / |xi|^2) L^T to 1e-6 of its largest entry (the fp32 rounding of the factor: each entry moves by
    at most 2^-24 relative, the product by twice that times P); the diagonal stays positive and the strict upper part
    is never written."""
    rng = np.random.default_rng(P)
    worst, signs = 0.0, set()
    for rep in range(300):
        L = _factor(rng, P, 100.0 if rep % 3 == 0 else 1.0)
        junk = np.triu(np.full((P, P), 7.0, np.float32), 1)
        xi = rng.standard_normal(8).astype(np.float32)
        al = float(rng.choice([0.0, 1.0, rng.uniform(0, 1)]))
        et = 1.0 if rep % 2 else float(rng.uniform(1e-4, 0.05))
        got, changed = _adapt(hc, L + junk, xi, al, et, AR.TARGET)
        want, want_changed = AR.adapt(L + junk, xi, al, et, AR.TARGET)
        assert changed is want_changed is True
        assert np.array_equal(SU.bits(np.tril(got)), SU.bits(want)), rep
        assert np.array_equal(np.triu(got, 1), junk)                          # never written
        assert np.array_equal(np.triu(want, 1), np.zeros((P, P), np.float32))
        assert (np.diag(got) > 0).all()
        d = et * (al - AR.TARGET)
        signs.add(d > 0)
        L64, x = L.astype(np.float64), xi[:P].astype(np.float64)
        ident = L64 @ (np.eye(P) + d * np.outer(x, x) / (x @ x)) @ L64.T
        G = np.tril(got).astype(np.float64)
        worst = max(worst, float(np.abs(G @ G.T - ident).max() / np.abs(ident).max()))
    assert signs == {True, False}
    assert worst <= 1e-6, worst


def test_guards_return_the_input_bits(hc):
    """xi = 0, d = 0 (alpha = target, or eta = 0), d not finite, a diagonal that is not positive, a downdate that
    reaches r2 <= 0 (|d| > 1, outside the kernel's range), an entry that overflows fp32 and a diagonal that underflows
    it: the factor comes back bit for bit, from the host build and from the restatement."""
    rng = np.random.default_rng(1)
    for P in (3, 4, 5):
        L = _factor(rng, P)
        xi = rng.standard_normal(8).astype(np.float32)
        e0 = np.zeros(8, np.float32)
        e0[0] = 1.0
        eye = np.eye(P, dtype=np.float32)
        neg = L.copy()
        neg[1, 1] = -neg[1, 1]
        zero = L.copy()
        zero[P - 1, P - 1] = 0.0
        tiny = eye.copy()
        tiny[0, 0] = np.float32(1.4e-45)                                     # the smallest subnormal
        huge = eye.copy()
        huge[0, 0] = np.float32(3e38)
        cases = [("xi = 0", L, np.zeros(8, np.float32), 1.0, 1.0, 0.234),
                 ("alpha = target", L, xi, 0.25, 1.0, 0.25), ("eta = 0", L, xi, 1.0, 0.0, 0.234),
                 ("d = nan", L, xi, NAN, 1.0, 0.234), ("d = inf", L, xi, 1.0, INF, 0.234),
                 ("a negative diagonal", neg, xi, 1.0, 1.0, 0.234), ("a zero diagonal", zero, xi, 0.0, 1.0, 0.234),
                 ("r2 <= 0", eye, e0, 0.0, 8.0, 0.5),                        # d = -4 along e_0
                 ("fp32 overflow", huge, e0, 1.0, 1.0, 0.0625),              # 3e38 sqrt(1.9375) > FLT_MAX
                 ("fp32 underflow", tiny, e0, 0.0, 1.0, 0.9375)]             # 1.4e-45 / 4 rounds to 0
        for name, F, z, al, et, target in cases:
            got, changed = _adapt(hc, F, z, al, et, target)
            want, want_changed = AR.adapt(F, z, al, et, target)
            assert not changed and not want_changed, name
            assert np.array_equal(SU.bits(got), SU.bits(F)), name
            assert np.array_equal(SU.bits(want), SU.bits(np.tril(F))), name


def test_guard_neighbours(hc):
    """A subnormal diagonal that survives the rounding is an update like any other."""
    eye = np.eye(3, dtype=np.float32)
    e0 = np.zeros(8, np.float32)
    e0[0] = 1.0
    tiny = eye.copy()
    tiny[0, 0] = np.float32(1.4e-44)
    got, changed = _adapt(hc, tiny, e0, 0.0, 1.0, 0.75)
    want, _ = AR.adapt(tiny, e0, 0.0, 1.0, 0.75)
    assert changed and np.array_equal(SU.bits(got), SU.bits(want)) and 0 < got[0, 0] < tiny[0, 0]


def test_alpha_at_its_cases(hc):
    """NaN (-inf against -inf, or a NaN estimate) -> 0; +inf (a chain at -inf meeting a finite proposal) -> 1; r >= 0
    -> 1; r < 0 -> exp(r) within 1e-13 relative; -inf (a dead proposal) -> 0."""
    for args, want in (((-INF, -INF, 0.0, 0.0), 0.0), ((NAN, -3.0, 0.0, 0.0), 0.0), ((-3.0, -3.0, NAN, 0.0), 0.0),
                       ((-3.0, -INF, 0.0, 0.0), 1.0), ((-3.0, -3.0, 0.0, 0.0), 1.0), ((-2.0, -3.0, -0.5, 0.0), 1.0),
                       ((-INF, -3.0, 0.0, 0.0), 0.0), ((-1e300, -3.0, 0.0, 0.0), 0.0)):
        assert hc.hc_mh_alpha(*args) == want == AR.alpha(*args), args
    rng = np.random.default_rng(2)
    for _ in range(3000):
        a = rng.normal(0, 3, 4) * rng.choice([1.0, 30.0])
        want = AR.alpha(*a)
        assert abs(hc.hc_mh_alpha(*a) - want) <= 1e-13 * want, a
    for r in (-1e-300, -1e-17, -0.5, -700.0):
        assert abs(hc.hc_mh_alpha(r, 0.0, 0.0, 0.0) - math.exp(r)) <= 1e-13 * math.exp(r)


def test_eta(hc):
    """eta = 1 at i = 0 and up to the last i with P (i + 1)^-gamma >= 1; below 1 and within 1e-13 relative of numpy's
    power from the first i where it leaves 1 (i + 1 > P^(1 / gamma): i = 9 for P = 3, 16 for P = 4, 25 for P = 5 at
    gamma = 1/2) up to 2^31 - 2."""
    for P, first in ((3, 9), (4, 16), (5, 25)):
        assert hc.hc_mh_eta(P, 0, 0.5) == 1.0 == AR.eta(P, 0, 0.5)
        assert hc.hc_mh_eta(P, first - 2, 0.5) == 1.0
        assert hc.hc_mh_eta(P, first, 0.5) < 1.0 and AR.eta(P, first, 0.5) < 1.0
        assert hc.hc_mh_eta(P, P - 1, 1.0) == 1.0 and hc.hc_mh_eta(P, P, 1.0) < 1.0
    rng = np.random.default_rng(3)
    for gamma in (0.5, 2.0 / 3.0, 1.0, 0.05):
        for i in list(range(200)) + [2 ** 31 - 2] + [int(v) for v in rng.integers(1, 2 ** 31 - 1, 300)]:
            for P in (3, 4, 5):
                want = AR.eta(P, i, gamma)
                assert abs(hc.hc_mh_eta(P, i, gamma) - want) <= 1e-13 * want, (P, i, gamma)


def test_batched_update_is_the_scalar_one():
    """adapt_batch (float64, the free-running reference's) against adapt() before its rounding: within fp32's."""
    rng = np.random.default_rng(4)
    for P in (3, 4):
        L = np.stack([_factor(rng, P) for _ in range(50)])
        xi = rng.standard_normal((50, P)).astype(np.float32)
        al = rng.uniform(0, 1, 50)
        got = AR.adapt_batch(L.astype(np.float64), xi.astype(np.float64), al, 0.3, AR.TARGET)
        for c in range(50):
            want, _ = AR.adapt(L[c], xi[c], al[c], 0.3, AR.TARGET)
            assert np.allclose(np.tril(got[c]), want, rtol=2e-7, atol=1e-9)


# ----------------------------------------------------------------------------------------------------------------
# the ABI and the refusals
# ----------------------------------------------------------------------------------------------------------------
def test_abi():
    from viforssms_amd import _lib
    for name, n_in in (("vissm_pmmh_adaptive", 7), ("vissm_sv_pmmh_adaptive", 6)):
        args = _lib.SIGNATURES[name][1]
        assert args[0] is _lib.SIGNATURES["vissm_pmmh"][1][0]                                      # one descriptor
        assert len(args) == 3 + n_in + 3 + 13 + 1
        assert args[3 + n_in:3 + n_in + 3] == [ctypes.c_int32, ctypes.c_double, ctypes.c_double]


NAMES = ["theta_cur", "ll_cur", "chol_in", "prior", "x_start", "obs", "obs_bin", "theta_chain", "ll_chain", "accept",
         "theta_end", "ll_end", "chol_end", "theta_prop", "ll_prop", "logu", "xi_trace", "alpha_trace", "eta_trace",
         "chol_trace"]


@pytest.mark.parametrize("sv", [False, True])
def test_library_refuses_without_gpu(sv):
    """Everything the adaptive entries refuse is host arithmetic before any GPU call: the twins' refusals, a bad
    adapt_end, target_accept or gamma, a null chol_in or chol_end."""
    from viforssms_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    A = ctypes.addressof(buf)
    names = [n for n in NAMES if not (sv and n == "obs_bin")]
    fn = lib.vissm_sv_pmmh_adaptive if sv else lib.vissm_pmmh_adaptive
    model = _lib.MODEL_SV if sv else _lib.MODEL_AR

    def call(desc, adapt_end=5, target=0.234, gamma=0.5, **null):
        ptrs = [None if null.get(n) else A for n in names]
        n_in = 6 if sv else 7
        return fn(ctypes.byref(desc) if desc is not None else None, 1, 0, *ptrs[:n_in], adapt_end, target, gamma,
                  *ptrs[n_in:], None)

    one = lambda **kw: _lib.PmmhDesc(**{**dict(model=model, C=1, N=64, n_iter=1, it0=0, T_total=4, dt=1.0,
                                               obs_std=1.0), **kw})
    assert call(None) == -1
    assert call(one(model=_lib.MODEL_AR if sv else _lib.MODEL_SV)) == -1 and b"SV" in lib.vissm_last_error()
    for kw in (dict(C=0), dict(N=96), dict(n_iter=-1), dict(it0=-1), dict(it0=2 ** 31 - 1), dict(T_total=-1)):
        assert call(one(**kw)) == -1, kw
    assert call(one(dt=0.0) if sv else one(obs_std=0.0)) == -1
    for end in (-1, -2 ** 31):
        assert call(one(), adapt_end=end) == -1 and b"adapt_end" in lib.vissm_last_error()
    for t in (0.0, 1.0, -0.1, 1.5, NAN, INF):
        assert call(one(), target=t) == -1 and b"target_accept" in lib.vissm_last_error(), t
    for g in (0.0, -0.5, 1.0000001, NAN, INF):
        assert call(one(), gamma=g) == -1 and b"gamma" in lib.vissm_last_error(), g
    for name in names[:-7]:                                      # the seven traces may be null
        assert call(one(), **{name: True}) == -1, name
        assert b"null pointer" in lib.vissm_last_error()
    if sv:
        for n in _lib.PF_PARTICLES:
            assert lib.vissm_sv_pmmh_adaptive_lds_bytes(n) == lib.vissm_sv_pmmh_lds_bytes(n) + 8 * (16 + 8) + 8 * 8
        assert lib.vissm_sv_pmmh_adaptive_lds_bytes(96) == 0
    else:
        for m, P in ((_lib.MODEL_AR, 3), (_lib.MODEL_LV, 3), (_lib.MODEL_FHN, 5)):
            assert _lib.MODEL_P[m] == P
            for n in _lib.PF_PARTICLES:
                assert lib.vissm_pmmh_adaptive_lds_bytes(m, n) == \
                    lib.vissm_pmmh_lds_bytes(m, n) + 8 * (P * P + 2 * P) + 8 * ((P * P + 1) // 2)
        assert lib.vissm_pmmh_adaptive_lds_bytes(_lib.MODEL_SV, 64) == 0
        assert lib.vissm_pmmh_adaptive_lds_bytes(_lib.MODEL_AR, 96) == 0


def test_python_refusals_without_gpu():
    """ops.pmmh_adaptive / ops.sv_pmmh_adaptive repeat the refusals as ValueError before they ask for a GPU tensor."""
    import torch
    from viforssms_amd import _lib, ops
    th, ll = torch.zeros(2, 3), torch.zeros(2, dtype=torch.float64)
    L, pr, x0, y = torch.eye(3).repeat(2, 1, 1), torch.ones(3, 2), torch.zeros(1), torch.zeros(1, 8)

    def run(model=SU.AR, theta=th, chol=L, N=64, n_iter=1, it0=0, adapt_end=1, **kw):
        return ops.pmmh_adaptive(model, theta, ll, chol, pr, x0, y, y, 1.0, 1.0, N, n_iter, 1, 0, adapt_end, it0=it0,
                                 **kw)

    th4, L4, pr4 = torch.zeros(2, 4), torch.eye(4).repeat(2, 1, 1), torch.ones(4, 2)

    def run_sv(theta=th4, chol=L4, N=64, n_iter=1, adapt_end=1, **kw):
        return ops.sv_pmmh_adaptive(theta, ll, chol, pr4, x0, torch.ones(9), 1.0, N, n_iter, 1, 0, adapt_end, **kw)

    with pytest.raises(ValueError, match="SV"):
        run(model=SU.SV)
    for f in (run, run_sv):
        with pytest.raises(ValueError, match="particles"):
            f(N=96)
        with pytest.raises(ValueError, match="iterations"):
            f(n_iter=-1)
        for end in (-1, 2 ** 31):
            with pytest.raises(ValueError, match="adapt_end"):
                f(adapt_end=end)
        for t in (0.0, 1.0, -0.1, NAN):
            with pytest.raises(ValueError, match="target_accept"):
                f(target_accept=t)
        for g in (0.0, 1.5, NAN):
            with pytest.raises(ValueError, match="gamma"):
                f(gamma=g)
        with pytest.raises(ValueError, match="theta_cur"):
            f(theta=torch.zeros(2, 7))
        with pytest.raises(_lib.VissmError, match="GPU only"):
            f()
    with pytest.raises(ValueError, match="chol_in"):
        run(chol=torch.eye(3))                                   # the twin's shared factor is not a factor per chain
    with pytest.raises(ValueError, match="chol_in"):
        run(chol=L.double())
    with pytest.raises(ValueError, match="chol_in"):
        run_sv(chol=torch.eye(4).repeat(3, 1, 1))


def test_product_refusals_without_gpu():
    """What theta_mcmc(adapt=True) and volatility_mcmc(adapt=True) refuse before they touch the device, on a stand-in
    that has only what those checks read."""
    from viforssms_amd import _lib
    from viforssms_amd.diagnostics import PosteriorDiagnostics

    class Stub(PosteriorDiagnostics):
        def __init__(self, model_id, family):
            self.mdef = types.SimpleNamespace(model_id=model_id, family=family)
            self.p_local, self.obs, self.filter_data = 8, np.linspace(1.0, 2.0, 21), (None, None, None)

        def target_len(self):
            return 20

    base = dict(n_chains=4, n_particles=64, n_iter=10, burn_in=4, adapt=True)
    for stub, fn in ((Stub(_lib.MODEL_AR, "ar"), "theta_mcmc"), (Stub(_lib.MODEL_SV, "sv"), "volatility_mcmc")):
        run = getattr(stub, fn)
        for kw, msg in ((dict(burn_in=0), "burn_in"), (dict(target_accept=0.0), "target_accept"),
                        (dict(target_accept=1.0), "target_accept"), (dict(target_accept=NAN), "target_accept"),
                        (dict(adapt_decay=0.0), "adapt_decay"), (dict(adapt_decay=1.5), "adapt_decay"),
                        (dict(adapt_decay=NAN), "adapt_decay"), (dict(n_particles=96), "n_particles"),
                        (dict(burn_in=10), "burn_in")):
            with pytest.raises(ValueError, match=msg):
                run(**{**base, **kw})
    with pytest.raises(ValueError, match="SV"):
        Stub(_lib.MODEL_SV, "sv").theta_mcmc(**base)
    with pytest.raises(ValueError, match="theta_mcmc"):
        Stub(_lib.MODEL_AR, "ar").volatility_mcmc(**base)


def test_cli_option():
    from viforssms_amd import config, sv
    base = ["hyperparameters.txt"]
    a = config.handle_opts(base + ["--mcmc", "8", "64", "100", "m.npz", "--mcmc-adapt"])
    assert a.mcmc == (8, 64, 100, "m.npz") and a.mcmc_adapt is True
    assert config.handle_opts(base + ["--mcmc", "8", "64", "100", "m.npz"]).mcmc_adapt is False
    assert config.handle_opts(base).mcmc_adapt is False
    with pytest.raises(SystemExit):
        config.handle_opts(base + ["--mcmc-adapt"])
    with pytest.raises(SystemExit):
        sv.run(["--mcmc-adapt"])


# ----------------------------------------------------------------------------------------------------------------
# the statistical conditions, for the reference alone
# ----------------------------------------------------------------------------------------------------------------
STAT_C, STAT_ITER, STAT_ADAPT, STAT_SCALE = 64, 5000, 3000, 100.0


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("case", MR.PRIOR_CASES)
def test_reference_meets_the_conditions(case, seed):
    """tests/test_gpu_pmmh_adapt.py's statistical test at its configuration, for the numpy adaptive chain on the exact
    Kalman likelihood of the AR fixture plus N(-1/2, 1) noise: 64 chains from the factor chol(D Sigma D), D =
    diag(100, 1, 1), adapting 3000 of 5000 iterations, the kept 2000 against the fixture's truth."""
    obs, obs_bin = PR.stat_case()
    t = MR.truth(case)
    rng = np.random.default_rng(100 + seed)
    r = AR.adaptive_chain(AR.exact_ar_loglik(MR.STAT_X0, obs, obs_bin, MR.STAT_OBS_STD, rng),
                          MR.stat_start(t, STAT_C, seed), AR.bad_factor(t["L"], STAT_SCALE), t["prior"], STAT_ITER,
                          STAT_ADAPT, rng)
    c = AR.stat_conditions(r["theta"][:, STAT_ADAPT:], r["accept"][:, STAT_ADAPT:], r["chol_end"], t)
    print(case, seed, c)
    assert c["ok"], c


def test_frozen_bad_factor_is_the_recorded_failure():
    """The control: with the bad factor frozen the same chain accepts under 2 % (the trial gave 0.2 - 0.3 %)."""
    obs, obs_bin = PR.stat_case()
    t = MR.truth("flat")
    rng = np.random.default_rng(7)
    r = AR.adaptive_chain(AR.exact_ar_loglik(MR.STAT_X0, obs, obs_bin, MR.STAT_OBS_STD, rng),
                          MR.stat_start(t, STAT_C, 1), AR.bad_factor(t["L"], STAT_SCALE), t["prior"], 500, 0, rng)
    assert r["accept"].mean() < 0.02
    assert np.array_equal(r["chol_end"][0], AR.bad_factor(t["L"], STAT_SCALE).astype(np.float64))
