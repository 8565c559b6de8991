"""The forecast's Euler-Maruyama steps on the host: viforssms_amd/csrc/sim_math.hpp, the code vissm_sde_simulate's
kernel runs, compiled for the CPU into libvissm_hostcheck.so (hc_sim_step, hc_sim_path), against a float64 numpy
restatement of the formulas (tests/sim_util.py); the death rule; the entry point's refusals, which run before any
device work; the ctypes mirror of VissmSimDesc.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

from tests import sim_util as SU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK = os.path.join(ROOT, "viforssms_amd", "libvissm_hostcheck.so")
FP = ctypes.POINTER(ctypes.c_float)


def _host():
    lib = ctypes.CDLL(HOSTCHECK)
    lib.hc_sim_step.restype = None
    lib.hc_sim_step.argtypes = [ctypes.c_int, FP, FP, ctypes.c_float, FP, FP]
    lib.hc_sim_path.restype = None
    lib.hc_sim_path.argtypes = [ctypes.c_int, FP, FP, ctypes.c_float, ctypes.c_float, ctypes.c_int, FP, FP, FP, FP]
    return lib


def _p(a):
    return a.ctypes.data_as(FP)


def _path(lib, model, x0, th, dt, normals, H, obs_std=None):
    S = SU.S_OF[model]
    x0, th, normals = (np.ascontiguousarray(a, dtype=np.float32) for a in (x0, th, normals))
    xo = np.full((S, H), -7.0, np.float32)
    yo = np.full((S, H), -7.0, np.float32)
    xe = np.full(S, -7.0, np.float32)
    lib.hc_sim_path(model, _p(x0), _p(th), dt, 0.0 if obs_std is None else obs_std, H, _p(normals), _p(xo),
                    _p(yo) if obs_std is not None else None, _p(xe))
    return xo, (yo if obs_std is not None else None), xe


@pytest.mark.parametrize("model", [SU.AR, SU.LV, SU.SV, SU.FHN])
def test_step_matches_float64_restatement(model):
    """One step, 64 random (x, theta, n) around the generators' true values.  Each output is a sum of at most four
    terms, each accurate to a few fp32 ulp of itself, so |got - ref| <= 16 * 2^-24 * sum|terms| with the term
    magnitudes from the float64 side."""
    lib = _host()
    rng = np.random.default_rng(100 + model)
    S, P, dt = SU.S_OF[model], SU.P_OF[model], SU.DT[model]
    x = (np.asarray(SU.TRUE_X[model]) * rng.uniform(0.7, 1.3, (64, S))).astype(np.float32)
    th = (np.asarray(SU.TRUE_THETA[model]) + rng.uniform(-0.1, 0.1, (64, P))).astype(np.float32)
    n = rng.standard_normal((64, 2)).astype(np.float32)
    terms = SU.step_terms(model, x.astype(np.float64), th.astype(np.float64), dt, n.astype(np.float64))
    worst = 0.0
    for i in range(64):
        out = np.zeros(2, np.float32)
        xi = np.zeros(2, np.float32)
        xi[:S] = x[i]
        thi = np.zeros(5, np.float32)
        thi[:P] = th[i]
        lib.hc_sim_step(model, _p(xi), _p(thi), dt, _p(n[i].copy()), _p(out))
        for d in range(S):
            ref = sum(float(t[i]) for t in terms[d])
            bound = 16.0 * 2.0 ** -24 * sum(abs(float(t[i])) for t in terms[d])
            assert len(terms[d]) <= 4
            worst = max(worst, abs(float(out[d]) - ref) / bound)
            assert abs(float(out[d]) - ref) <= bound, (model, i, d, out[d], ref, bound)
    print(f"model {model}: largest |got - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("model,obs_std", [(SU.AR, None), (SU.AR, 0.5), (SU.LV, 1.0), (SU.SV, None), (SU.FHN, 0.1)])
@pytest.mark.parametrize("H", [0, 1, 9])
def test_path_is_the_step_chained(model, obs_std, H):
    """hc_sim_path = hc_sim_step applied H times to its own output, observations x + obs_std n from the step's
    second group of normals, x_end the last state (the start for H = 0)."""
    lib = _host()
    rng = np.random.default_rng(7)
    S, P, dt = SU.S_OF[model], SU.P_OF[model], SU.DT[model]
    NS = 2 * S if obs_std is not None else S
    x0 = np.asarray(SU.TRUE_X[model], np.float32)
    th = np.zeros(5, np.float32)
    th[:P] = SU.TRUE_THETA[model]
    nn = rng.standard_normal((H, NS)).astype(np.float32)
    xo, yo, xe = _path(lib, model, x0, th, dt, nn, H, obs_std)
    cur = np.zeros(2, np.float32)
    cur[:S] = x0
    for t in range(H):
        nxt = np.zeros(2, np.float32)
        nt = np.zeros(2, np.float32)
        nt[:S] = nn[t, :S]
        lib.hc_sim_step(model, _p(cur), _p(th), dt, _p(nt), _p(nxt))
        cur = nxt
        assert np.array_equal(xo[:, t], cur[:S])
        if obs_std is not None:
            assert np.array_equal(yo[:, t], cur[:S] + np.float32(obs_std) * nn[t, S:])
    assert np.array_equal(xe, cur[:S])


def test_dead_rows_are_nan_from_the_dying_step_on():
    lib = _host()
    th = np.asarray(SU.TRUE_THETA[SU.LV], np.float32)
    H = 8
    nn = np.zeros((H, 4), np.float32)
    nn[3, 0] = -40.0          # step 3 throws x1 far below zero
    x0 = np.asarray([0.5, 100.0], np.float32)
    xo, yo, xe = _path(lib, SU.LV, x0, th, 0.1, nn, H, obs_std=1.0)
    assert np.isfinite(xo[:, :3]).all() and np.isfinite(yo[:, :3]).all() and (xo[:, :3] > 0).all()
    assert np.isnan(xo[:, 3:]).all() and np.isnan(yo[:, 3:]).all() and np.isnan(xe).all()
    # the float64 replay dies at the same step
    ref = SU.replay(SU.LV, x0[None], th[None], 0.1, nn.reshape(1, -1), H, obs_std=1.0)
    assert ref[-1][0] == 3
    assert np.allclose(xo[:, :3], ref[0][0][:, :3], rtol=1e-5)
    # theta not finite: every step's state is NaN
    bad = th.copy()
    bad[1] = np.inf
    xo, _, xe = _path(lib, SU.LV, np.asarray([100.0, 100.0], np.float32), bad, 0.1, nn[:, :2].copy(), H)
    assert np.isnan(xo).all() and np.isnan(xe).all()
    xo, _, xe = _path(lib, SU.FHN, np.asarray([0.5, 0.5], np.float32),
                      np.asarray([np.nan, 1.0, 1.5, 0.0, 0.0], np.float32), 0.1, nn[:, :2].copy(), H)
    assert np.isnan(xo).all() and np.isnan(xe).all()
    # a start outside the domain (LV: a non-positive coordinate; any model: not finite): NaN throughout
    for model, start in [(SU.LV, [-1.0, 100.0]), (SU.LV, [0.0, 100.0]), (SU.LV, [np.nan, 100.0]),
                         (SU.AR, [np.inf]), (SU.SV, [1.0, np.nan])]:
        P = SU.P_OF[model]
        t = np.zeros(5, np.float32)
        t[:P] = SU.TRUE_THETA[model]
        xo, _, xe = _path(lib, model, np.asarray(start, np.float32), t, 0.1, np.zeros((H, 2), np.float32), H)
        assert np.isnan(xo).all() and np.isnan(xe).all(), (model, start)
    # AR has no boundary: a negative state lives
    t = np.zeros(5, np.float32)
    t[:3] = SU.TRUE_THETA[SU.AR]
    xo, _, _ = _path(lib, SU.AR, np.asarray([-3.0], np.float32), t, 1.0, np.zeros((H, 1), np.float32), H)
    assert np.isfinite(xo).all()


def test_simulate_refuses_bad_arguments_without_gpu():
    """vissm_sde_simulate checks its descriptor and pointers before any device work."""
    from viforssms_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(16)   # never dereferenced: the checks run first

    def call(model=_lib.MODEL_LV, B=4, H=8, t0=0, n_stream=None, with_obs=0, theta=fake, xs=fake, x=fake, y=None,
             xe=fake):
        S = _lib.MODEL_S.get(model, 1)
        ns = (2 * S if with_obs else S) if n_stream is None else n_stream
        d = _lib.SimDesc(model, B, H, t0, ns, 0.1, 1.0, with_obs)
        rc = lib.vissm_sde_simulate(ctypes.byref(d), 1, 0, theta, xs, x, y, xe, None)
        return rc, lib.vissm_last_error()

    for kw, msg in [(dict(model=4), b"unknown model"), (dict(model=-1), b"unknown model"),
                    (dict(B=-1), b"bad shape"), (dict(H=-1), b"bad shape"), (dict(t0=-1), b"bad shape"),
                    (dict(model=_lib.MODEL_SV, with_obs=1, y=fake), b"SV"),
                    (dict(with_obs=1, y=None), b"null pointer"),
                    (dict(theta=None), b"null pointer"), (dict(xs=None), b"null pointer"),
                    (dict(x=None), b"null pointer"), (dict(xe=None), b"null pointer"),
                    (dict(n_stream=4), b"n_stream"), (dict(n_stream=2, with_obs=1, y=fake), b"n_stream"),
                    (dict(model=_lib.MODEL_AR, n_stream=2), b"n_stream"), (dict(n_stream=0), b"n_stream"),
                    (dict(H=2 ** 30, t0=2 ** 30), b"2^31"), (dict(with_obs=2, y=fake), b"with_obs")]:
        rc, err = call(**kw)
        assert rc < 0 and msg in err, (kw, rc, err)
    assert lib.vissm_sde_simulate(None, 1, 0, fake, fake, fake, None, fake, None) < 0
    # no samples: nothing to launch, whatever the pointers point to
    assert call(B=0)[0] == 0
    assert _lib.SIM_TILE == 64 and _lib.MODEL_S == SU.S_OF and _lib.MODEL_P == SU.P_OF


def test_sim_desc_layout_matches_ctypes():
    """The ctypes mirror of VissmSimDesc has the C compiler's size and last-field offset, and the header's constants
    are the module's (in the manner of tests/test_lib.py::test_abi_struct_layouts_match_ctypes)."""
    import re
    from viforssms_amd import _lib
    lib = ctypes.CDLL(HOSTCHECK)
    f = lib.vissm_host_abi_layout
    f.restype = None
    f.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]
    out = (ctypes.c_size_t * 2)()
    f(5, out)
    assert out[0] == ctypes.sizeof(_lib.SimDesc) == 32
    assert out[1] == _lib.SimDesc.with_obs.offset == 28
    assert [n for n, _ in _lib.SimDesc._fields_] == ["model", "B", "H", "t0", "n_stream", "dt", "obs_std", "with_obs"]
    header = open(os.path.join(ROOT, "include", "vissm.h")).read()
    assert int(re.search(r"#define VISSM_SIM_TILE (\d+)", header).group(1)) == _lib.SIM_TILE
