"""Particle marginal Metropolis-Hastings without a GPU: csrc/mh_math.hpp (the code the kernel runs, built for the host
in libvissm_hostcheck.so) against the numpy restatement of tests/pmmh_ref.py; the library's and ops.pmmh's refusals,
which are host arithmetic; the ABI; split-R-hat on a case worked by hand; the command-line option; and the statistical
bars of tests/test_gpu_pmmh.py for the numpy reference alone."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import pf_ref as PR
from tests import pmmh_ref as MR
from tests import sim_util as SU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK = os.path.join(ROOT, "viforssms_amd", "libvissm_hostcheck.so")
FP = ctypes.POINTER(ctypes.c_float)
INF = float("inf")


@pytest.fixture(scope="module")
def hc():
    lib = ctypes.CDLL(HOSTCHECK)
    u32, u64, d, i = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_double, ctypes.c_int
    lib.hc_mh_row.restype, lib.hc_mh_row.argtypes = u64, [u64] * 5
    lib.hc_mh_words.restype, lib.hc_mh_words.argtypes = None, [u32, u64, u64, ctypes.POINTER(u32)]
    lib.hc_mh_uniform.restype, lib.hc_mh_uniform.argtypes = d, [u32]
    lib.hc_mh_log_uniform.restype, lib.hc_mh_log_uniform.argtypes = d, [u32]
    lib.hc_mh_xi.restype, lib.hc_mh_xi.argtypes = None, [u64, u64, FP]
    lib.hc_mh_propose.restype, lib.hc_mh_propose.argtypes = None, [FP, FP, FP, i, FP]
    lib.hc_mh_log_prior.restype, lib.hc_mh_log_prior.argtypes = d, [FP, FP, i]
    lib.hc_mh_accept.restype, lib.hc_mh_accept.argtypes = i, [d] * 5
    return lib


def _p(a):
    return a.ctypes.data_as(FP)


ROWS = [(0x0123456789ABCDEF, 0), (7, 2 ** 32 - 3), (2 ** 64 - 1, 2 ** 63 + 12345), (99, 2 ** 64 - 64)]


@pytest.mark.parametrize("seed,row0", ROWS)
def test_words_uniform_and_normals_bitwise(hc, seed, row0):
    """The row of (i, c), the three Philox blocks, u, and the eight normals of box_muller4_ref: bit for bit."""
    for i, C, c, N in ((0, 1, 0, 64), (3, 5, 2, 64), (1000, 64, 63, 1024), (2 ** 31 - 2, 3, 1, 128)):
        r = MR.row_of(row0, i, C, c, N)
        assert hc.hc_mh_row(row0, i, C, c, N) == r
        for g in range(3):
            out = (ctypes.c_uint32 * 4)()
            hc.hc_mh_words(g, r, seed, out)
            assert list(out) == [int(v) for v in MR.words(seed, r, g)]
        x = int(MR.words(seed, r, 2)[0])
        u = hc.hc_mh_uniform(x)
        assert u == MR.uniform(x) and 0.0 < u < 1.0
        assert abs(hc.hc_mh_log_uniform(x) - math.log(u)) <= 2 * np.spacing(abs(math.log(u)))
        got = np.zeros(8, np.float32)
        hc.hc_mh_xi(r, seed, _p(got))
        assert np.array_equal(SU.bits(got), SU.bits(MR.xi(seed, r)))
    for x in (0, 0xFF, 0x100, 0xFFFFFF00, 0xFFFFFFFF):
        assert hc.hc_mh_uniform(x) == MR.uniform(x) == ((x >> 8) + 0.5) / 2 ** 24


@pytest.mark.parametrize("P", [3, 5])
def test_proposal_and_log_prior(hc, P):
    """theta' within 1 ulp fp32 of the float64 sum (it is that sum, rounded once) and lp exact, on random inputs and on
    a factor with an upper triangle the sum must not read."""
    rng = np.random.default_rng(P)
    for rep in range(200):
        th = rng.normal(0, 3, P).astype(np.float32)
        L = np.tril(rng.normal(0, 0.3, (P, P))).astype(np.float32)
        if rep % 2:
            L = (L + np.triu(np.full((P, P), 1e6, np.float32), 1)).astype(np.float32)
        z = rng.standard_normal(8).astype(np.float32)
        prior = np.stack([rng.normal(0, 2, P), rng.uniform(0.1, 10, P)], 1).astype(np.float32)
        out = np.zeros(P, np.float32)
        hc.hc_mh_propose(_p(th), _p(np.ascontiguousarray(L)), _p(z), P, _p(out))
        want = MR.propose(th, L, z)
        assert np.all(np.abs(out.astype(np.float64) - want) <= np.spacing(np.abs(want))), (out, want)
        assert np.array_equal(SU.bits(out), SU.bits(want))
        assert hc.hc_mh_log_prior(_p(th), _p(np.ascontiguousarray(prior)), P) == MR.log_prior(th, prior)


RECORDED = [  # (logu, ll', ll, lp', lp) -> accept
    ((-1.0, -3.0, -3.0, -0.5, 0.0), True), ((-0.5, -3.0, -3.0, -0.5, 0.0), False),
    ((-0.5, -3.0, -3.0, -0.5, -0.0), False), ((-1e-9, -100.0, -100.0, 0.0, 0.0), True),
    ((-1.0, -INF, -3.0, 0.0, 0.0), False),        # a dead proposal
    ((-30.0, -1e300, -INF, 0.0, 0.0), True),      # a chain at -inf accepts any finite proposal
    ((-1.0, -INF, -INF, 0.0, 0.0), False),        # -inf against -inf: NaN
    ((-1.0, float("nan"), -3.0, 0.0, 0.0), False), ((-1.0, -3.0, -3.0, float("nan"), 0.0), False),
    ((-0.75, -64.25, -64.0, -1.5, -1.0), False),   # equality is a rejection
    ((-0.7500000000000001, -64.25, -64.0, -1.5, -1.0), True),
]


def test_decision_on_recorded_inputs(hc):
    for args, want in RECORDED:
        assert bool(hc.hc_mh_accept(*args)) is want is MR.accept(*args), args
    rng = np.random.default_rng(5)
    for _ in range(2000):
        a = rng.normal(0, 2, 5)
        a[0] = -abs(a[0])
        assert bool(hc.hc_mh_accept(*a)) is MR.accept(*a)


def test_replay_follows_the_decisions():
    """pmmh_ref.replay on a hand-made run: reject, accept, dead proposal."""
    prior = np.array([[0.0, 1.0]] * 3, np.float32)
    th0 = np.zeros((1, 3), np.float32)
    prop = np.array([[[1, 0, 0], [0.5, 0, 0], [0.1, 0, 0]]], np.float32)
    ll_prop = np.array([[-10.0, -9.9, -INF]])
    logu = np.array([[-0.1, -0.1, -5.0]])
    th, ll, acc, cur = MR.replay(th0, np.array([-10.0]), prior, prop, ll_prop, logu)
    assert acc.tolist() == [[0, 1, 0]]                # -0.5 < -0.1 fails; 0.1 - 0.125 = -0.025 > -0.1; dead
    assert th[0].tolist() == [[0, 0, 0], [0.5, 0, 0], [0.5, 0, 0]] and ll[0].tolist() == [-10.0, -9.9, -9.9]
    assert cur[0].tolist() == [[0, 0, 0], [0, 0, 0], [0.5, 0, 0]]


def test_abi():
    from viforssms_amd import _lib
    lib = ctypes.CDLL(HOSTCHECK)
    out = (ctypes.c_size_t * 2)()
    lib.vissm_host_abi_layout.restype = None
    lib.vissm_host_abi_layout(8, out)
    assert out[0] == ctypes.sizeof(_lib.PmmhDesc) == 32 and out[1] == _lib.PmmhDesc.obs_std.offset == 28
    assert [f[0] for f in _lib.PmmhDesc._fields_] == ["model", "C", "N", "n_iter", "it0", "T_total", "dt", "obs_std"]
    assert len(_lib.SIGNATURES["vissm_pmmh"][1]) == 3 + 15 + 1


def test_library_refuses_without_gpu():
    """Everything vissm_pmmh refuses is host arithmetic before any GPU call: with every pointer a dummy a bad
    descriptor comes back VISSM_EINVAL."""
    from viforssms_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    A = ctypes.addressof(buf)
    names = ["theta_cur", "ll_cur", "prop_chol", "prior", "x_start", "obs", "obs_bin", "theta_chain", "ll_chain",
             "accept", "theta_end", "ll_end", "theta_prop", "ll_prop", "logu"]

    def call(desc, **null):
        ptrs = [None if null.get(n) else A for n in names]
        return lib.vissm_pmmh(ctypes.byref(desc) if desc is not None else None, 1, 0, *ptrs, None)

    bad = lambda **kw: _lib.PmmhDesc(**{**dict(model=_lib.MODEL_AR, C=0, N=64, n_iter=1, it0=0, T_total=4, dt=1.0,
                                               obs_std=1.0), **kw})
    assert call(bad()) == -1 and b"chains" in lib.vissm_last_error()          # C < 1 refuses what follows too
    one = lambda **kw: bad(**{**dict(C=1), **kw})
    assert call(one(model=_lib.MODEL_SV)) == -1 and b"SV" in lib.vissm_last_error()
    assert call(one(model=7)) == -1 and call(one(model=-1)) == -1
    for sd in (0.0, -1.0, float("nan"), INF, -INF):
        assert call(one(obs_std=sd)) == -1, sd
        assert b"obs_std" in lib.vissm_last_error()
    for n in (0, 1, 32, 63, 96, 100, 2048, -64):
        assert call(one(N=n)) == -1, n
        assert b"particles" in lib.vissm_last_error()
    for c in (0, -1, -2 ** 31):
        assert call(one(C=c)) == -1, c
    for kw in (dict(n_iter=-1), dict(it0=-1), dict(it0=2 ** 31 - 1, n_iter=1), dict(T_total=-1)):
        assert call(one(**kw)) == -1, kw
    assert call(one(model=_lib.MODEL_LV, T_total=2 ** 30)) == -1 and b"2^31" in lib.vissm_last_error()
    assert call(one(model=_lib.MODEL_FHN, T_total=2 ** 31 - 1)) == -1
    assert call(None) == -1
    for name in names[:12]:
        assert call(one(), **{name: True}) == -1, name
        assert b"null pointer" in lib.vissm_last_error()
    for model, S in ((_lib.MODEL_AR, 1), (_lib.MODEL_LV, 2), (_lib.MODEL_FHN, 2)):
        for n in _lib.PF_PARTICLES:
            assert lib.vissm_pmmh_lds_bytes(model, n) == 8 * n + 4 * S * n + 192
    assert lib.vissm_pmmh_lds_bytes(_lib.MODEL_SV, 64) == 0 and lib.vissm_pmmh_lds_bytes(_lib.MODEL_AR, 96) == 0


def test_python_refusals_without_gpu():
    """ops.pmmh repeats the refusals as ValueError before it asks for a GPU tensor."""
    import torch
    from viforssms_amd import _lib, ops
    th, ll = torch.zeros(2, 3), torch.zeros(2, dtype=torch.float64)
    L, pr, x0, y = torch.eye(3), torch.ones(3, 2), torch.zeros(1), torch.zeros(1, 8)

    def run(model=SU.AR, theta=th, obs=y, obs_std=1.0, N=64, n_iter=1, it0=0, row0=0):
        return ops.pmmh(model, theta, ll, L, pr, x0, obs, obs, 1.0, obs_std, N, n_iter, 1, row0, it0=it0)

    with pytest.raises(ValueError, match="SV"):
        run(model=SU.SV)
    with pytest.raises(ValueError, match="unknown model"):
        run(model=9)
    for sd in (0.0, -1.0, float("nan"), INF):
        with pytest.raises(ValueError, match="obs_std"):
            run(obs_std=sd)
    for n in (0, 32, 96, 2048):
        with pytest.raises(ValueError, match="particles"):
            run(N=n)
    with pytest.raises(ValueError, match="theta_cur"):
        run(theta=torch.zeros(0, 3))
    with pytest.raises(ValueError, match="theta_cur"):
        run(theta=torch.zeros(2, 4))
    for kw in (dict(n_iter=-1), dict(it0=-1), dict(it0=2 ** 31 - 1)):
        with pytest.raises(ValueError, match="iterations"):
            run(**kw)
    with pytest.raises(ValueError, match="2\\^31"):
        run(obs=torch.zeros(1, 1).expand(1, 2 ** 31))
    with pytest.raises(ValueError, match="row0"):
        run(row0=-1)
    with pytest.raises(_lib.VissmError, match="GPU only"):
        run()


def test_split_rhat_by_hand():
    """Two chains of four draws: halves (1, 2), (3, 4), (2, 3), (4, 5); W = 1/2, the half means 1.5, 3.5, 2.5, 4.5 have
    variance 5/3, B = 10/3, so R-hat = sqrt((W / 2 + B / 2) / W) = sqrt(23 / 6)."""
    from viforssms_amd.diagnostics import split_rhat
    x = np.array([[1.0, 2, 3, 4], [2, 3, 4, 5]])
    assert abs(split_rhat(x) - math.sqrt(23.0 / 6.0)) < 1e-14 and abs(MR.split_rhat(x) - math.sqrt(23.0 / 6.0)) < 1e-14
    odd = np.array([[1.0, 2, 9, 3, 4], [2, 3, 9, 4, 5]])                       # the middle draw is dropped
    assert abs(split_rhat(odd) - math.sqrt(23.0 / 6.0)) < 1e-14
    rng = np.random.default_rng(0)
    iid = rng.standard_normal((8, 2000))
    assert abs(split_rhat(iid) - 1.0) < 0.01 and abs(split_rhat(iid) - MR.split_rhat(iid)) < 1e-12
    assert split_rhat(iid + np.arange(8)[:, None]) > 2.0                        # chains that disagree
    assert math.isnan(split_rhat(np.zeros((2, 3)))) and math.isnan(split_rhat(np.ones((2, 8))))


def test_cli_option():
    from viforssms_amd import config
    base = ["hyperparameters.txt"]
    assert config.handle_opts(base + ["--mcmc", "8", "64", "100", "m.npz"]).mcmc == (8, 64, 100, "m.npz")
    assert config.handle_opts(base).mcmc is None
    for bad in (["--mcmc", "0", "64", "100", "m.npz"], ["--mcmc", "8", "96", "100", "m.npz"],
                ["--mcmc", "8", "64", "1", "m.npz"], ["--mcmc", "eight", "64", "100", "m.npz"],
                ["--mcmc", "8", "64", "m.npz"]):
        with pytest.raises(SystemExit):
            config.handle_opts(base + bad)


def test_batched_kalman_is_the_scalar_one():
    obs, obs_bin = PR.stat_case()
    rng = np.random.default_rng(3)
    th = np.asarray(SU.TRUE_THETA[SU.AR]) + rng.normal(0, 0.2, (5, 3))
    got = MR.kalman_ar_loglik_batch(th, 10.0, obs[0], obs_bin[0], 1.0)
    want = [PR.kalman_ar_loglik(t, 10.0, obs[0], obs_bin[0], 1.0) for t in th]
    assert np.allclose(got, want, rtol=1e-13, atol=0)


# ----------------------------------------------------------------------------------------------------------------
# the statistical bars, for the reference alone
# ----------------------------------------------------------------------------------------------------------------
REF_ITER, REF_BURN = 250, 50


@pytest.mark.parametrize("case", MR.PRIOR_CASES)
def test_reference_meets_its_own_bars(case):
    """AR fixture, C = 64 chains of the numpy PMMH reference at N = 64 against the exact chain's truth.  250
    iterations, the first 50 dropped: the chains start spread as the posterior, so the burn-in only has to forget the
    approximation, and 64 x 200 draws at an autocorrelation time near 20 leave about 600 effective draws: the sd ratio
    has a standard error near 3 %.  (The GPU test runs 1500 / 300; at 0.12 s per iteration of the numpy filter
    that would take this file six minutes.)"""
    obs, obs_bin = PR.stat_case()
    t = MR.truth(case)
    rng = np.random.default_rng(11)
    r = MR.pmmh_chain(SU.AR, MR.stat_start(t, 64, 1).astype(np.float64), t["L"], t["prior"], [MR.STAT_X0], obs, obs_bin,
                      1.0, MR.STAT_OBS_STD, 64, REF_ITER, rng)
    s = MR.summarise(r["theta"][:, REF_BURN:], r["accept"][:, REF_BURN:])
    bars = MR.stat_bars(s, t)
    print(case, {k: np.round(v, 4) for k, v in s.items()}, bars)
    assert bars["ok"], bars
    if case == "informative":   # the case exists because a chain that drops the prior passes the flat one
        flat = MR.truth("flat")
        assert abs(t["mean"][0] - flat["mean"][0]) > 40 * math.hypot(t["se"][0], s["se"][0])
