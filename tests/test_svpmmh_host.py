"""Particle marginal Metropolis-Hastings for the stochastic-volatility model without a GPU: one whole iteration run
serially by the host build (hc_svpmmh_iteration, libvissm_hostcheck.so: mh_math.hpp and svf::filter_step, the code the
kernel runs) against the numpy restatement of tests/svpmmh_ref.py; the refusals of the library, of ops.sv_pmmh and of
volatility_mcmc, which are host arithmetic; the command-line option; the batched grid log-likelihood against
svf_ref.grid_pass; the fixture's own assertions re-checked from what it stores; and the statistical bars of
tests/test_gpu_svpmmh.py for the numpy reference alone."""
import ctypes
import math
import os
import types

import numpy as np
import pytest

from tests import pf_ref as PR
from tests import pmmh_ref as MR
from tests import sim_util as SU
from tests import svf_ref as SR
from tests import svpmmh_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK = os.path.join(ROOT, "viforssms_amd", "libvissm_hostcheck.so")
FP = ctypes.POINTER(ctypes.c_float)
INF = float("inf")


@pytest.fixture(scope="module")
def hc():
    lib = ctypes.CDLL(HOSTCHECK)
    u64, d, i, f, v = ctypes.c_uint64, ctypes.c_double, ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    lib.hc_svpmmh_iteration.restype = i
    lib.hc_svpmmh_iteration.argtypes = [u64] * 5 + [i, i, f, FP, d, FP, FP, f, FP, FP, ctypes.POINTER(d)] + [v] * 6
    lib.hc_svf_move.restype = f
    lib.hc_svf_move.argtypes = [f, FP, f, f]
    return lib


def _p(a):
    return a.ctypes.data_as(FP)


def _iteration(hc, seed, row0, i, C, c, n, th, ll, L, prior, h0, y, dt=1.0):
    T = len(y) - 1
    tr = {"h": np.full((T + 1, n), np.nan, np.float32), "q": np.zeros((T, n), np.uint64),
          "anc": np.full((T, n), -2, np.int32), "n": np.zeros((T, n), np.float32), "m": np.zeros(T, np.float32),
          "W": np.zeros(T, np.uint64)}
    thp, out = np.zeros(4, np.float32), (ctypes.c_double * 4)()
    acc = hc.hc_svpmmh_iteration(seed, row0, i, C, c, n, T, dt, _p(th), ll, _p(np.ascontiguousarray(L)),
                                 _p(np.ascontiguousarray(prior)), h0, _p(y), _p(thp), out,
                                 *(tr[k].ctypes.data for k in ("h", "q", "anc", "n", "m", "W")))
    return acc, thp, dict(lp=out[0], lpp=out[1], logu=out[2], llp=out[3]), tr


CASES = [(0x0123456789ABCDEF, 0, 0, 1, 0, 64, 1), (7, 2 ** 32 - 3, 3, 5, 2, 64, 5),
         (2 ** 64 - 1, 2 ** 63 + 12345, 9, 3, 1, 128, 9), (99, 2 ** 64 - 64, 2, 64, 63, 64, 21)]


@pytest.mark.parametrize("seed,row0,i,C,c,n,T", CASES)
def test_host_iteration_against_the_numpy_replay(hc, seed, row0, i, C, c, n, T):
    """theta', lp, lp' and the decision exact (log u within 2 ulp of math.log, as tests/test_pmmh_host.py holds it);
    every filter step under tests/test_svf_host.py's bars: the weights within the q bar of the float64 weights, the
    ancestors exactly the Python-int resampling of the step's own weights with the contract's integer U, each new h the
    bitwise move of its ancestor's with the traced normal, the normals the Philox stream's (counter (t / 4, 0, row),
    entry t % 4, Box-Muller in float64); ll' the sum of the increments."""
    from tests import philox_ref
    rng = np.random.default_rng(T + n)
    th = (np.asarray(SR.PARAM_INIT) + rng.uniform(-0.1, 0.1, 4)).astype(np.float32)
    L = np.tril(rng.normal(0, 0.02, (4, 4))).astype(np.float32)
    prior = VR.stat_prior()
    y, _ = SR.simulate_series(T, SR.PARAM_INIT, 1.0, SR.FIX_H0, 1.0, rng)
    ll_cur = -3.0
    acc, thp, o, tr = _iteration(hc, seed, row0, i, C, c, n, th, ll_cur, L, prior, SR.FIX_H0, y)
    r, want, lpp, lu = VR.iteration(seed, row0, i, C, c, n, th, L, prior)
    assert np.array_equal(SU.bits(thp), SU.bits(want))
    assert o["lp"] == MR.log_prior(th, prior) and o["lpp"] == lpp == MR.log_prior(thp, prior)
    assert abs(o["logu"] - lu) <= 2 * np.spacing(abs(lu))
    assert bool(acc) is MR.accept(o["logu"], o["llp"], ll_cur, o["lpp"], o["lp"])
    assert np.all(tr["h"][0] == np.float32(SR.FIX_H0))
    ll = 0.0
    th64 = thp.astype(np.float64)
    for t in range(T):
        h, q = tr["h"][t], tr["q"][t]
        U = SU.resample_u(seed, t, r)
        want_anc, W = PR.systematic_ints(q, int(U))
        assert W == int(tr["W"][t]) > 0 and tr["anc"][t].tolist() == want_anc and int(q.max()) == 1 << 40
        alive, lw64, m64, qref = SR.weigh(h.astype(np.float64), y[t], y[t + 1], th64, 1.0)
        lw32 = SR.state_logw(h, y[t], y[t + 1], thp, 1.0, np.float32).astype(np.float64)
        d = 8.0 * max(float(np.max(np.abs(lw32 - lw64))), 2.0 ** -20 * float(np.mean(np.abs(lw64))))
        qr = qref.astype(np.float64)
        tol = qr * (math.expm1(2.0 * d) + (np.abs(lw64 - m64) + 2.0) * 2.0 ** -23) + 1.0
        assert alive.all() and np.all(np.abs(q.astype(np.float64) - qr) <= tol)
        rows = [(r + p) & MR.M64 for p in range(n)]
        ctr = np.array([[t >> 2, 0, row & 0xFFFFFFFF, row >> 32] for row in rows], np.uint64)
        w = np.stack([philox_ref.philox4x32_10(list(cc), [seed & 0xFFFFFFFF, seed >> 32]) for cc in ctr])
        nn = philox_ref.box_muller(philox_ref.uniforms(w), np.float64).reshape(n, 4)[:, t & 3].astype(np.float32)
        assert np.array_equal(SU.bits(tr["n"][t]), SU.bits(nn))
        for j in range(n):
            moved = np.float32(hc.hc_svf_move(h[tr["anc"][t, j]], _p(thp), 1.0, tr["n"][t, j]))
            assert SU.bits(np.array([moved]))[0] == SU.bits(tr["h"][t + 1, j:j + 1])[0], (t, j)
        ll += float(tr["m"][t]) + math.log(W) - 40.0 * math.log(2.0) - math.log(n)
    assert abs(o["llp"] - ll) <= 1e-12 * max(1.0, abs(ll))


def test_host_iteration_death_and_minus_infinity(hc):
    th = np.asarray(SR.PARAM_INIT, np.float32)
    L, prior = np.zeros((4, 4), np.float32), VR.stat_prior()
    y, _ = SR.simulate_series(12, SR.PARAM_INIT, 1.0, SR.FIX_H0, 1.0, np.random.default_rng(3))
    args = (5, 1000, 2, 3, 1, 64, th)
    acc, thp, o, _ = _iteration(hc, *args, -INF, L, prior, SR.FIX_H0, y)
    assert acc == 1 and np.array_equal(thp, th) and math.isfinite(o["llp"])   # a chain at -inf takes a live proposal
    for series, h0 in ((np.where(np.arange(13) == 6, np.float32(0), y), SR.FIX_H0),
                       (np.where(np.arange(13) == 6, np.float32(1e30), y), SR.FIX_H0), (y, float("nan")), (y, INF)):
        acc, _, o, tr = _iteration(hc, *args, -3.0, L, prior, h0, np.ascontiguousarray(series, np.float32))
        assert acc == 0 and o["llp"] == -INF
        assert _iteration(hc, *args, -INF, L, prior, h0, np.ascontiguousarray(series, np.float32))[0] == 0   # NaN
    acc, _, o, _ = _iteration(hc, *args, -3.0, L, prior, SR.FIX_H0, y[:1])     # T = 0
    assert o["llp"] == 0.0 and acc == 1


# ----------------------------------------------------------------------------------------------------------------
# refusals: host arithmetic before any GPU call
# ----------------------------------------------------------------------------------------------------------------
def test_abi():
    from viforssms_amd import _lib
    assert _lib.SIGNATURES["vissm_sv_pmmh"][1][0] is _lib.SIGNATURES["vissm_pmmh"][1][0]       # one descriptor
    assert len(_lib.SIGNATURES["vissm_sv_pmmh"][1]) == 3 + 14 + 1


def test_library_refuses_without_gpu():
    from viforssms_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    A = ctypes.addressof(buf)
    names = ["theta_cur", "ll_cur", "prop_chol", "prior", "h_start", "obs", "theta_chain", "ll_chain", "accept",
             "theta_end", "ll_end", "theta_prop", "ll_prop", "logu"]

    def call(desc, **null):
        ptrs = [None if null.get(n) else A for n in names]
        return lib.vissm_sv_pmmh(ctypes.byref(desc) if desc is not None else None, 1, 0, *ptrs, None)

    bad = lambda **kw: _lib.PmmhDesc(**{**dict(model=_lib.MODEL_SV, C=0, N=64, n_iter=1, it0=0, T_total=4, dt=1.0,
                                               obs_std=0.0), **kw})
    assert call(bad()) == -1 and b"chains" in lib.vissm_last_error()          # C < 1 refuses what follows too
    one = lambda **kw: bad(**{**dict(C=1), **kw})
    assert call(None) == -1 and b"null descriptor" in lib.vissm_last_error()
    for model in (_lib.MODEL_AR, _lib.MODEL_LV, _lib.MODEL_FHN, 7, -1):
        assert call(one(model=model)) == -1 and b"SV" in lib.vissm_last_error()
    for sd in (0.0, -1.0, float("nan"), INF, 5.0):                            # obs_std is ignored
        assert call(one(obs_std=sd, C=0)) == -1 and b"chains" in lib.vissm_last_error()
    for n in (0, 1, 32, 63, 96, 100, 2048, -64):
        assert call(one(N=n)) == -1, n
        assert b"particles" in lib.vissm_last_error()
    for c in (0, -1, -2 ** 31):
        assert call(one(C=c)) == -1, c
    for kw in (dict(n_iter=-1), dict(it0=-1), dict(it0=2 ** 31 - 1, n_iter=1), dict(it0=2 ** 30, n_iter=2 ** 30)):
        assert call(one(**kw)) == -1 and b"iterations" in lib.vissm_last_error(), kw
    for t in (-1, 2 ** 31 - 1):
        assert call(one(T_total=t)) == -1 and b"T_total" in lib.vissm_last_error(), t
    for dt in (0.0, -1.0, float("nan"), INF, -INF):
        assert call(one(dt=dt)) == -1 and b"dt" in lib.vissm_last_error(), dt
    for name in names[:11]:
        assert call(one(), **{name: True}) == -1, name
        assert b"null pointer" in lib.vissm_last_error()
    for n in _lib.PF_PARTICLES:
        assert lib.vissm_sv_pmmh_lds_bytes(n) == 8 * n + 4 * n + 192 == lib.vissm_pmmh_lds_bytes(_lib.MODEL_AR, n)
    for n in (0, 1, 63, 96, 2048, -64):
        assert lib.vissm_sv_pmmh_lds_bytes(n) == 0
    # the existing entry still refuses SV, with its message
    assert lib.vissm_pmmh(ctypes.byref(one()), 1, 0, *([A] * 15), None) == -1
    assert b"no observation model for SV" in lib.vissm_last_error()
    assert lib.vissm_pmmh_lds_bytes(_lib.MODEL_SV, 64) == 0


def test_python_refusals_without_gpu():
    """ops.sv_pmmh repeats the refusals as ValueError before it asks for a GPU tensor; ops.pmmh still refuses SV."""
    import torch
    from viforssms_amd import _lib, ops
    th, ll = torch.zeros(2, 4), torch.zeros(2, dtype=torch.float64)
    L, pr, h0, y = torch.eye(4), torch.ones(4, 2), torch.zeros(1), torch.ones(9)

    def run(theta=th, obs=y, dt=1.0, N=64, n_iter=1, it0=0, row0=0):
        return ops.sv_pmmh(theta, ll, L, pr, h0, obs, dt, N, n_iter, 1, row0, it0=it0)

    for n in (0, 32, 96, 2048):
        with pytest.raises(ValueError, match="particles"):
            run(N=n)
    for dt in (0.0, -1.0, float("nan"), INF):
        with pytest.raises(ValueError, match="dt"):
            run(dt=dt)
    for bad in (torch.zeros(0, 4), torch.zeros(2, 3), torch.zeros(4)):
        with pytest.raises(ValueError, match="theta_cur"):
            run(theta=bad)
    for kw in (dict(n_iter=-1), dict(it0=-1), dict(it0=2 ** 31 - 1)):
        with pytest.raises(ValueError, match="iterations"):
            run(**kw)
    for bad in (torch.ones(1, 9), torch.ones(0), torch.ones(9, dtype=torch.float64)):
        with pytest.raises(ValueError, match="obs"):
            run(obs=bad)
    with pytest.raises(ValueError, match="2\\^31"):
        run(obs=torch.ones(1).expand(2 ** 31))
    with pytest.raises(ValueError, match="row0"):
        run(row0=-1)
    with pytest.raises(_lib.VissmError, match="GPU only"):
        run()
    with pytest.raises(ValueError, match="SV"):
        ops.pmmh(SU.SV, th, ll, L, pr, h0, y[None], y[None], 1.0, 1.0, 64, 1, 1, 0)


def test_product_refusals_without_gpu():
    """What volatility_mcmc refuses before it touches the device, on a stand-in that has only what those checks read."""
    from viforssms_amd import _lib
    from viforssms_amd.diagnostics import PosteriorDiagnostics

    class Stub(PosteriorDiagnostics):
        def __init__(self, model_id, family, obs):
            self.mdef = types.SimpleNamespace(model_id=model_id, family=family)
            self.p_local, self.obs, self.filter_data = 8, obs, None

        def target_len(self):
            return len(self.obs) - 1

    y = np.linspace(1.0, 2.0, 21)
    with pytest.raises(ValueError, match="theta_mcmc"):
        Stub(_lib.MODEL_AR, "ar", y).volatility_mcmc(4, 64, 10, 2)
    sv = Stub(_lib.MODEL_SV, "sv", y)
    base = dict(n_chains=4, n_particles=64, n_iter=10, burn_in=2)
    for kw, msg in ((dict(n_particles=96), "n_particles"), (dict(n_chains=0), "n_chains"), (dict(n_chains=9), "n_chains"),
                    (dict(burn_in=10), "burn_in"), (dict(burn_in=-1), "burn_in"), (dict(step_scale=0.0), "step_scale"),
                    (dict(step_scale=INF), "step_scale"), (dict(step_scale=float("nan")), "step_scale")):
        with pytest.raises(ValueError, match=msg):
            sv.volatility_mcmc(**{**base, **kw})
    for t, v, what in ((7, 0.0, "= 0"), (19, 0.0, "= 0"), (5, np.nan, "finite"), (20, np.inf, "finite")):
        bad = y.copy()
        bad[t] = v
        with pytest.raises(ValueError, match=what):
            Stub(_lib.MODEL_SV, "sv", bad).volatility_mcmc(**base)
    with pytest.raises(ValueError, match="SV"):                    # the existing method still refuses SV
        sv.theta_mcmc(4, 64, 10, 2)


def test_cli_option():
    from viforssms_amd import sv
    for bad in (["--mcmc", "0", "64", "100", "m.npz"], ["--mcmc", "8", "96", "100", "m.npz"],
                ["--mcmc", "8", "64", "1", "m.npz"], ["--mcmc", "eight", "64", "100", "m.npz"],
                ["--mcmc", "8", "64", "m.npz"]):
        with pytest.raises(SystemExit):
            sv.run(bad)


# ----------------------------------------------------------------------------------------------------------------
# the grid truth and the fixture
# ----------------------------------------------------------------------------------------------------------------
def test_batched_grid_is_the_scalar_one():
    y = VR.stat_series()
    rng = np.random.default_rng(3)
    th = np.asarray(SR.PARAM_INIT) + rng.normal(0, 1, (5, 4)) * np.asarray(VR.PRIOR_SD)
    for n_grid, lo, hi in ((313, -24.0, 2.0), (201, -16.0, 1.0)):
        got = VR.grid_loglik_batch(th, SR.FIX_H0, y, SR.FIX_DT, n_grid, lo, hi)
        want = [SR.grid_pass(t, SR.FIX_H0, y, SR.FIX_DT, n_grid, lo, hi)["loglik"] for t in th]
        assert np.allclose(got, want, rtol=1e-13, atol=0)
    at_init = VR.grid_loglik_batch(np.asarray([SR.PARAM_INIT]), SR.FIX_H0, y, SR.FIX_DT)[0]
    assert abs(at_init - SR.fixture_truth()[0]) <= 1e-6                      # the filter fixture's own value


def test_fixture_sanity():
    """The generator's assertions from what it stored: the three grids agree to 1e-6 on 256 of the exact chain's kept
    draws (a sample of them is evaluated again here), every split-R-hat is at most 1.05; the factor and the prior are
    what the generator states; the reference's acceptance at N = 64 lies below the exact chain's."""
    from tests.golden import make_svpmmh_fixture as G
    with np.load(VR.FIXTURE) as z:
        f = {k: z[k] for k in z.files}
    assert f["check_theta"].shape == (256, 4) and f["check_ll"].shape == (3, 256)
    assert np.isfinite(f["check_ll"]).all() and np.abs(f["check_ll"] - f["check_ll"][0]).max() <= 1e-6
    y = VR.stat_series()
    for k, grid in enumerate(VR.GRID_CHECKS):
        again = VR.grid_loglik_batch(f["check_theta"][:8], SR.FIX_H0, y, SR.FIX_DT, *grid)
        assert np.allclose(again, f["check_ll"][k, :8], rtol=1e-12, atol=0)
    assert f["rhat"].shape == (4,) and np.all(f["rhat"] <= 1.05) and np.all(f["rhat"] > 0.99)
    assert np.array_equal(f["L"], G.factor()) and f["L"].dtype == np.float32
    assert np.array_equal(f["prior"], VR.stat_prior()) and np.array_equal(f["start"], np.asarray(G.PILOT_MEAN, np.float32))
    for k in ("mean", "sd", "se", "ref64_mean", "ref64_sd", "ref64_se"):
        assert f[k].shape == (4,) and np.isfinite(f[k]).all()
    assert 0.1 < float(f["ref64_acc"]) < float(f["acc"]) < 0.5
    # the reference at N = 64 meets the exact chain's mean and sd (PMMH is exact for any N) but not its acceptance
    s = {k: f[f"ref64_{k}"] for k in ("mean", "sd", "se")}
    s["acc"], s["acc_se"] = float(f["ref64_acc"]), float(f["ref64_acc_se"])
    bars = MR.stat_bars(s, VR.truth("exact"))
    assert np.all(bars["dmean_over_se"] <= 4.0) and np.all(np.abs(bars["sd_ratio"] - 1.0) <= 0.1)
    assert bars["dacc_over_se"] > 4.0 and MR.stat_bars(s, VR.truth("ref64"))["ok"]


# ----------------------------------------------------------------------------------------------------------------
# the statistical bars, for the reference alone
# ----------------------------------------------------------------------------------------------------------------
REF_ITER, REF_BURN = 250, 50


def test_reference_meets_its_own_bars():
    """SV fixture, C = 64 chains of the numpy PMMH reference at N = 64: mean and sd against the exact chain's truth,
    acceptance against the stored reference run at the same N.  250 iterations, the first 50 dropped, as
    tests/test_pmmh_host.py runs its own: the chains start spread as the posterior, so the burn-in only has to forget
    the approximation."""
    t = VR.truth("ref64")
    rng = np.random.default_rng(11)
    r = VR.pmmh_chain(VR.stat_start(t, 64, 1).astype(np.float64), t["L"], t["prior"], SR.FIX_H0, VR.stat_series(),
                      SR.FIX_DT, 64, REF_ITER, rng)
    s = MR.summarise(r["theta"][:, REF_BURN:], r["accept"][:, REF_BURN:])
    bars = MR.stat_bars(s, t)
    print({k: np.round(v, 4) for k, v in s.items()}, bars)
    assert bars["ok"], bars
