"""vissm_sv_filter_sorted (ops.sv_filter_sorted) on the GPU.

Teacher-forced, step by step, from the kernel's own traces: the sorted array of every step is the sort of the states
before it, bit for bit (tests/cpm_ref.py: -0 before +0, dead particles last); the resampling integer is the contract's
within one unit; the ancestors are the Python-int resampling (tests/pf_ref.py) of the traced weights and integer,
exactly; the weights, the increments and the moved states sit within tests/test_gpu_svfilter.py's bars of the float64
reference applied to the traced sorted states.  The start states mix negatives, positives, +-0, duplicates and NaN: the
model's own h is always negative and would hide a sign error in the sort key.  Repeated launches and a sub-batch are
compared bitwise, a zero in y kills the filter, and the noise of ll(aux') - ll(aux) -- what the chain's acceptance ratio
sees -- meets the numpy reference's at rho = 0.99 and rho = 0."""
import itertools
import os

import numpy as np
import pytest
import torch

from tests import cpm_ref as CR
from tests import pf_ref as PR
from tests import svf_ref as R
from tests.sim_util import PF_ONE as ONE, bits as _bits, state_bar as _bar
from tests.test_gpu_svfilter import _q_tol

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 1.0
KEYS = ("loglik", "ll_inc", "cloud", "sorted", "q", "anc", "u")


def g(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def pack_n(un):
    """Move normals [K, T, N] -> the entry's layout [K, G, N, 4], the tail words 0."""
    K, T, N = un.shape
    G = (T + 3) // 4
    pad = np.zeros((K, 4 * G, N), np.float32)
    pad[:, :T] = un
    return np.ascontiguousarray(pad.reshape(K, G, 4, N).transpose(0, 1, 3, 2))


def unpack_n(aux_n, T):
    """The entry's layout [K, G, N, 4] -> move normals [K, T, N]."""
    K, G, N, _ = aux_n.shape
    return np.ascontiguousarray(aux_n.transpose(0, 1, 3, 2).reshape(K, 4 * G, N)[:, :T])


def _run(th, h0, y, N, un, ur, cloud=True, trace=True):
    from viforssms_amd import ops
    r = ops.sv_filter_sorted(g(th), g(h0), g(y), DT, N, g(pack_n(un)), g(ur), cloud=cloud, trace=trace)
    torch.cuda.synchronize()
    c = lambda t: None if t is None else t.cpu().numpy()
    return {"loglik": c(r.loglik), "ll_inc": c(r.ll_inc), "cloud": c(r.cloud), "sorted": c(r.sorted_trace),
            "q": c(r.q_trace), "anc": c(r.anc_trace), "u": c(r.u_trace)}


def _same(a, b, keys=KEYS):
    for k in keys:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def _inputs(K, N, T, rng):
    """theta within 0.1 of PARAM_INIT, a series simulated at PARAM_INIT, fresh normals, and start states spread over
    [-12, 3] with +-0, duplicates and NaN among them."""
    th = (np.asarray(R.PARAM_INIT) + rng.uniform(-0.1, 0.1, (K, 4))).astype(np.float32)
    y, _ = R.simulate_series(T, R.PARAM_INIT, DT, R.FIX_H0, 1.0, rng)
    h0 = rng.uniform(-12.0, 3.0, (K, N)).astype(np.float32)
    h0[:, 1], h0[:, 5], h0[:, 9], h0[:, 17] = 0.0, -0.0, 0.0, -0.0
    h0[:, 20:24] = h0[:, 30:31]                      # duplicates
    h0[:, 40], h0[:, 3] = np.nan, np.nan
    un, ur = rng.standard_normal((K, T, N)).astype(np.float32), rng.standard_normal((K, T)).astype(np.float32)
    return th, h0.reshape(-1), y, un, ur


@pytest.mark.parametrize("K,N,T", list(itertools.product((1, 3), (64, 128, 1024), (1, 63, 65))) + [(1, 256, 5),
                                                                                                   (1, 512, 5)])
def test_teacher_forced(K, N, T):
    """N = 64 has no exchange through LDS, 128 the first one, 1024 all ten; T = 65 has a last group of one word."""
    rng = np.random.default_rng(10 * N + T + K)
    th, h0, y, un, ur = _inputs(K, N, T, rng)
    r = _run(th, h0, y, N, un, ur)
    cloud, srt, anc, q = r["cloud"], r["sorted"], r["anc"].astype(np.int64), r["q"]
    assert cloud.shape == srt.shape == q.shape == (K, T, N) and r["u"].shape == (K, T)
    assert np.isfinite(cloud).all() and np.isfinite(r["loglik"]).all()
    u_want = CR.resample_u(ur)
    assert np.abs(r["u"].astype(np.int64) - u_want).max() <= 1
    th64 = th.astype(np.float64)
    exp64, exp32 = np.empty((K * N, 1, T)), np.empty((K * N, 1, T), np.float32)
    prev = h0.reshape(K, N)
    shares = {"q": 0.0, "ll_inc": 0.0}
    for t in range(T):
        assert np.array_equal(_bits(srt[:, t]), _bits(CR.sort_states(prev))), t
        for k in range(K):
            s = srt[k, t]
            alive, lw64, m64, qref = R.weigh(s.astype(np.float64), y[t], y[t + 1], th64[k], DT)
            assert alive.sum() == (N - 2 if t == 0 else N)
            lw32 = R.state_logw(s, y[t], y[t + 1], th[k], DT, np.float32).astype(np.float64)
            qk = [int(v) for v in q[k, t]]
            want_anc, W = PR.systematic_ints(qk, int(r["u"][k, t]))
            assert W > 0 and max(qk) == ONE
            assert anc[k, t].tolist() == want_anc, (k, t)
            tol = _q_tol(qref, lw64, lw32, m64, alive)
            err = np.abs(np.asarray(qk, np.float64) - qref.astype(np.float64))
            assert np.all(err <= tol), (k, t, float(np.max(err / tol)))
            shares["q"] = max(shares["q"], float(np.max(err / tol)))
            v = PR.ll_increment(m64, W, N)
            bar = 8.0 * max(float(np.max(np.abs(lw32 - lw64)[alive])), 2.0 ** -20 * abs(v))
            assert abs(float(r["ll_inc"][k, t]) - v) <= bar, (k, t)
            shares["ll_inc"] = max(shares["ll_inc"], abs(float(r["ll_inc"][k, t]) - v) / bar)
        ha = np.take_along_axis(srt[:, t], anc[:, t], axis=1)
        exp64[:, 0, t] = R.h_step(ha.astype(np.float64), th64[:, None, :], DT, un[:, t].astype(np.float64)).reshape(-1)
        exp32[:, 0, t] = R.h_step(ha, th[:, None, :], DT, un[:, t], np.float32).reshape(-1)
        prev = cloud[:, t]
    bar, e32 = _bar(exp64, exp32)
    dev = np.abs(cloud.transpose(0, 2, 1).reshape(K * N, 1, T) - exp64)
    print(f"K {K} N {N} T {T}: e32 {e32:.3e}, shares of the bars: cloud {np.max(dev / bar):.3f} q {shares['q']:.3f} "
          f"ll_inc {shares['ll_inc']:.3f}")
    assert np.all(dev <= bar)
    # loglik is the ordered double sum of the increments, of which ll_inc keeps the fp32 rounding: half an ulp each
    inc = r["ll_inc"].astype(np.float64)
    slack = 0.5 * np.spacing(np.abs(r["ll_inc"])).astype(np.float64).sum(1) + 1e-12
    assert np.all(np.abs(r["loglik"] - np.cumsum(inc, 1)[:, -1]) <= slack)


@pytest.mark.parametrize("N", [64, 128, 1024])
def test_bitwise_repeat_untraced_and_sub_batch(N):
    K, T = 3, 65
    th, h0, y, un, ur = _inputs(K, N, T, np.random.default_rng(31 + N))
    full = _run(th, h0, y, N, un, ur)
    _same(full, _run(th, h0, y, N, un, ur))
    plain = _run(th, h0, y, N, un, ur, cloud=False, trace=False)
    assert plain["cloud"] is None and plain["q"] is None
    _same(full, plain, ("loglik", "ll_inc"))
    one = _run(th[2:3], h0[2 * N:], y, N, un[2:3], ur[2:3])
    for k in KEYS:
        assert np.array_equal(_bits(one[k][0]), _bits(full[k][2])), k


def test_a_zero_in_y_kills_the_filter():
    K, N, T = 2, 128, 20
    th, h0, y, un, ur = _inputs(K, N, T, np.random.default_rng(5))
    y = y.copy()
    y[9] = 0.0                                       # step 9 divides by it: NaN weights, W = 0
    r = _run(th, h0, y, N, un, ur)
    assert np.all(r["loglik"] == -np.inf)
    assert np.isfinite(r["ll_inc"][:, :9]).all() and np.isnan(r["ll_inc"][:, 9:]).all()
    assert np.isfinite(r["cloud"][:, :9]).all() and np.isnan(r["cloud"][:, 9:]).all()
    assert np.all(r["q"][:, 9:] == 0)
    h_nan = np.full(K * N, np.nan, np.float32)       # every particle dead at the start
    assert np.all(_run(th, h_nan, y, N, un, ur)["loglik"] == -np.inf)


def test_fresh_aux_layout():
    """cpm_fresh_aux: half 0 holds normal_base's rows in the entry's layout, half 1 and aux_sel are zero."""
    from viforssms_amd import ops
    C, T, N, seed, row0 = 3, 65, 64, 77, 2 ** 32 - 100
    aux_n, aux_r, aux_sel = ops.cpm_fresh_aux(C, T, N, seed, row0, DEV)
    G = ops.cpm_groups(T)
    assert aux_n.shape == (C, 2, G, N, 4) and aux_r.shape == (C, 2, T) and aux_sel.shape == (C,)
    assert not aux_n[:, 1].any() and not aux_r[:, 1].any() and not aux_sel.any() and aux_sel.dtype == torch.int32
    eps = ops.normal_base(seed, row0, C * N, T, 1, DEV)[0].cpu().numpy().reshape(C, N, T)
    assert np.array_equal(_bits(aux_n[:, 0].cpu().numpy()), _bits(pack_n(eps.transpose(0, 2, 1))))
    epr = ops.normal_base(seed, row0 + C * N, C, T, 1, DEV)[0].cpu().numpy()
    assert np.array_equal(_bits(aux_r[:, 0].cpu().numpy()), _bits(epr))


def test_ratio_noise_meets_the_reference():
    """The first 257 values of the fitted series, theta = PARAM_INIT, N = 64, K = 256 filters: the sd of D = ll(aux') -
    ll(aux), aux' = numpy cn of aux and fresh normals, lies within the project's sd bar [0.8, 1.25] of the numpy
    reference's at the same shape (another seed: with 256 draws 4 se of the ratio is about 25 %), at rho = 0.99 and at
    rho = 0; and sd_0.99 / sd_0 is at most 1.5 times the reference's ratio."""
    y = CR.noise_series(ROOT)
    K, N = CR.NOISE_K, CR.NOISE_N
    th = np.tile(np.asarray(R.PARAM_INIT, np.float32), (K, 1))
    h0 = np.array([CR.NOISE_H0], np.float32)
    ll = lambda un, ur: _run(th, h0, y, N, un, ur, cloud=False, trace=False)["loglik"]
    got = {rho: CR.ratio_noise(ll, rho, 3) for rho in (0.99, 0.0)}
    ref = {rho: CR.reference_ratio_noise(ROOT, rho, 1) for rho in (0.99, 0.0)}
    print("sd(D): kernel", got, "reference", ref)
    for rho in (0.99, 0.0):
        assert 0.8 <= got[rho] / ref[rho] <= 1.25, rho
    assert got[0.99] / got[0.0] <= 1.5 * ref[0.99] / ref[0.0]
