"""vissm_sv_cpmmh (ops.sv_cpmmh; volatility_mcmc(correlation=...)) on the GPU.

Replay: the traced proposals, log u and decisions are checked as tests/test_gpu_svpmmh.py checks the twin's (the host
restatement from the chain's previous state, a factor of small rows); the proposal's move normals are numpy's cn of the
half the proposal was made from and ops.normal_base's rows, bit for bit, its resampling normals cn of the float64
Box-Muller within the gap tests/test_gpu_noise.py allows the hardware transcendentals; the proposal's estimate is
ops.sv_filter_sorted on the proposal's aux, bit for bit; aux_sel is the parity of the accepts.  Chained, repeated,
untraced and single-chain launches are compared bitwise, aux and chol_end included; dead proposals leave the chain and
its aux_sel where they were; the adaptive factor replays from its traces and a frozen chain is the fixed one.  The
chains' draws meet the exact (grid) posterior of the SV fixture, acceptance included, which the ordinary kernel at
N = 64 cannot.  Then the product path."""
import itertools
import os

import numpy as np
import pytest
import torch

from tests import cpm_ref as CR
from tests import philox_ref
from tests import pmmh_adapt_ref as AR
from tests import pmmh_ref as MR
from tests import svf_ref as SR
from tests import svpmmh_ref as VR
from tests.sim_util import PF_SEED as SEED, bits as _bits
from tests.test_gpu_noise import _bar as _noise_bar
from tests.test_gpu_sv_sorted import pack_n, unpack_n
from tests.test_gpu_svpmmh import MCMC_KEYS, _setup, _ulps32

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT, P, RHO = 1.0, VR.P, 0.99
KEYS = ("theta_chain", "ll_chain", "accept", "theta_end", "ll_end", "theta_prop", "ll_prop", "logu", "chol_end",
        "xi_trace", "alpha_trace", "eta_trace", "chol_trace")
AUX_SEED = SEED + 5


def g(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _fresh(C, T, N, row0=1 << 40):
    from viforssms_amd import ops
    return ops.cpm_fresh_aux(C, T, N, AUX_SEED, row0, DEV)


def _clone(aux):
    return tuple(a.clone() for a in aux)


def _sorted_ll(th, h0, y, N, aux_n, aux_r):
    """ops.sv_filter_sorted's loglik on one half per filter: aux_n [K, G, N, 4], aux_r [K, T] (torch)."""
    from viforssms_amd import ops
    return ops.sv_filter_sorted(g(th), g(np.array([h0], np.float32)), g(y), DT, N, aux_n.contiguous(),
                                aux_r.contiguous()).loglik.cpu().numpy()


def _run(th, ll, chol, prior, h0, y, N, n_iter, row0, aux, rho=RHO, it0=0, trace=True, adapt_end=0, seed=SEED):
    """The launch mutates aux (three torch tensors); the result also holds copies of them after it."""
    from viforssms_amd import ops
    chol = np.asarray(chol, np.float32)
    if chol.ndim == 2:
        chol = np.repeat(chol[None], len(th), 0)
    r = ops.sv_cpmmh(g(th), g(np.asarray(ll, np.float64)), g(chol), g(prior), g(np.array([h0], np.float32)), g(y), DT, N,
                     n_iter, seed, row0, rho, *aux, adapt_end=adapt_end, target_accept=AR.TARGET, gamma=AR.GAMMA,
                     it0=it0, trace=trace)
    torch.cuda.synchronize()
    assert r.aux_sel is aux[2]
    out = {k: (None if getattr(r, k) is None else getattr(r, k).cpu().numpy()) for k in KEYS}
    out.update(aux_n=aux[0].cpu().numpy(), aux_r=aux[1].cpu().numpy(), aux_sel=aux[2].cpu().numpy())
    return out


def _same(a, b, keys):
    for k in keys:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def _eps_r(seed, frow, T):
    """The first Box-Muller output (float64) of the Philox blocks (t, 1, lo32(frow), hi32(frow)), t < T."""
    ctr = np.zeros((T, 4), np.uint64)
    ctr[:, 0], ctr[:, 1] = np.arange(T), 1
    ctr[:, 2], ctr[:, 3] = frow & 0xFFFFFFFF, frow >> 32
    w = philox_ref.philox4x32_10(ctr, np.asarray([seed & 0xFFFFFFFF, seed >> 32], np.uint64))
    return philox_ref.box_muller(philox_ref.uniforms(w), np.float64).reshape(T, 4)[:, 0]


CHAIN = ("theta_chain", "ll_chain", "accept", "theta_prop", "ll_prop", "logu")


@pytest.mark.parametrize("N,C,n_iter,T", list(itertools.product((64, 128, 1024), (1, 3), (1, 5), (1, 63, 65))) +
                         [(256, 3, 5, 65), (512, 1, 1, 5)])
def test_replay(N, C, n_iter, T):
    from viforssms_amd import ops
    th, y, prior, L = _setup(C, T, 1000 * N + 100 * C + 10 * n_iter + T)
    h0, base = SR.FIX_H0, 11 + 5 * N
    aux = _fresh(C, T, N)
    ll0 = _sorted_ll(th, h0, y, N, aux[0][:, 0], aux[1][:, 0])
    r = _run(th, ll0, L, prior, h0, y, N, n_iter, base, aux)
    th_chain, ll_chain, acc, cur = MR.replay(th, ll0, prior, r["theta_prop"], r["ll_prop"], r["logu"])
    worst_t = worst_u = 0.0
    for c in range(C):
        for i in range(n_iter):
            _, want, _, lu = VR.iteration(SEED, base, i, C, c, N, cur[c, i], L, prior)
            worst_t = max(worst_t, float(_ulps32(r["theta_prop"][c, i], want).max()))
            worst_u = max(worst_u, abs(r["logu"][c, i] - lu) / np.spacing(abs(lu)))
    assert worst_t <= 1.0 and worst_u <= 2.0
    assert np.isfinite(r["ll_prop"]).all(), "the stable-range inputs left the domain"
    assert np.array_equal(r["accept"], acc)
    assert np.array_equal(_bits(r["theta_chain"]), _bits(th_chain))
    assert np.array_equal(_bits(r["ll_chain"]), _bits(ll_chain))
    assert np.array_equal(_bits(r["theta_end"]), _bits(th_chain[:, -1]))
    assert np.array_equal(_bits(r["ll_end"]), _bits(ll_chain[:, -1]))
    assert np.array_equal(r["aux_sel"], acc.sum(1) % 2)
    # The last iteration's proposal sits in the half aux_sel names if it was accepted, in the other if not; the half
    # it was made from is the other one either way, and the last iteration did not write it.
    i = n_iter - 1
    new = np.where(acc[:, i] == 1, r["aux_sel"], 1 - r["aux_sel"])
    ci = np.arange(C)
    un_new, un_old = r["aux_n"][ci, new], r["aux_n"][ci, 1 - new]
    ur_new, ur_old = r["aux_r"][ci, new], r["aux_r"][ci, 1 - new]
    eps = ops.normal_base(SEED, base + i * C * N, C * N, T, 1, DEV)[0].cpu().numpy().reshape(C, N, T)
    want_n = pack_n(CR.cn(unpack_n(un_old, T), eps.transpose(0, 2, 1), RHO))   # (the last group's tail words: 0)
    assert np.array_equal(_bits(un_new), _bits(want_n))
    sigma = float(CR.sigma_of(RHO))
    worst_r = 0.0
    for c in range(C):
        want_r = CR.cn(ur_old[c], _eps_r(SEED, MR.row_of(base, i, C, c, N), T).astype(np.float32), RHO)
        tol = sigma * _noise_bar() + np.spacing(np.abs(want_r)).astype(np.float64)
        dev = np.abs(ur_new[c].astype(np.float64) - want_r.astype(np.float64))
        worst_r = max(worst_r, float(np.max(dev / tol)))
    ll_want = _sorted_ll(r["theta_prop"][:, i], h0, y, N, g(un_new), g(ur_new))
    print(f"N {N} C {C} n_iter {n_iter} T {T}: theta_prop {worst_t:.2f} ulp, logu {worst_u:.2f} ulp, ur' {worst_r:.3f} "
          f"of its bar, accepted {int(acc.sum())} of {C * n_iter}")
    assert worst_r <= 1.0
    assert np.array_equal(_bits(r["ll_prop"][:, i]), _bits(ll_want))


@pytest.mark.parametrize("N,T", [(64, 65), (1024, 63), (128, 5)])
def test_chaining_repeat_and_independence_of_the_block(N, T):
    """3 + 2 iterations chained through theta_end / ll_end / chol_end and the same aux tensors are the five of one
    launch, aux included; two launches on cloned aux agree; without the traces the outputs are the same; chain 2 of
    three is reproduced by single-chain launches on its rows and its slice of aux."""
    C = 3
    th, y, prior, L = _setup(C, T, 7 + N)
    L = (L * 20.0).astype(np.float32)               # steps wide enough for both decisions to occur
    h0, row0 = SR.FIX_H0, 12345
    aux0 = _fresh(C, T, N)
    ll0 = _sorted_ll(th, h0, y, N, aux0[0][:, 0], aux0[1][:, 0])
    full = _run(th, ll0, L, prior, h0, y, N, 5, row0, _clone(aux0))
    print(f"N {N} T {T}: accepted {int(full['accept'].sum())} of {5 * C}")
    everything = KEYS[:9] + ("aux_n", "aux_r", "aux_sel")
    _same(full, _run(th, ll0, L, prior, h0, y, N, 5, row0, _clone(aux0)), everything)
    plain = _run(th, ll0, L, prior, h0, y, N, 5, row0, _clone(aux0), trace=False)
    assert plain["theta_prop"] is None and plain["xi_trace"] is None
    _same(full, plain, KEYS[:5] + ("chol_end", "aux_n", "aux_r", "aux_sel"))
    aux = _clone(aux0)
    a = _run(th, ll0, L, prior, h0, y, N, 3, row0, aux)
    b = _run(a["theta_end"], a["ll_end"], a["chol_end"], prior, h0, y, N, 2, row0, aux, it0=3)
    for k in CHAIN:
        assert np.array_equal(_bits(np.concatenate([a[k], b[k]], 1)), _bits(full[k])), k
    _same(b, full, ("theta_end", "ll_end", "chol_end", "aux_sel"))
    # the half each chain holds at the end is the same; the other half holds the last rejected or replaced proposal
    _same(b, full, ("aux_n", "aux_r"))
    c, t, ll = 2, th[2:3], ll0[2:3]
    one_aux = tuple(x[c:c + 1].clone() for x in aux0)
    for i in range(5):
        # a single chain at it0 = i sits on row0' + i N: place it on row0 + (3 i + 2) N
        one = _run(t, ll, L, prior, h0, y, N, 1, row0 + (3 * i + c) * N - i * N, one_aux, it0=i)
        for k in CHAIN:
            assert np.array_equal(_bits(one[k][0, 0]), _bits(full[k][c, i])), (k, i)
        t, ll = one["theta_end"], one["ll_end"]
    for k in ("aux_n", "aux_r", "aux_sel"):
        assert np.array_equal(_bits(one[k][0]), _bits(full[k][c])), k


def test_dead_proposals_and_a_chain_entering_at_minus_infinity():
    """A zero inside y, a value 1e30 away and a start that is not finite kill every proposal's filter: nothing is
    accepted, theta, ll and aux_sel stay.  A chain entering at ll = -inf takes its first finite proposal."""
    C, N, T = 3, 128, 20
    th, y, prior, L = _setup(C, T, 5)
    h0 = SR.FIX_H0
    far, zero = y.copy(), y.copy()
    far[7], zero[9] = 1e30, 0.0
    ll0 = np.array([-5.0, -6.0, -7.0])
    aux0 = _fresh(C, T, N)
    aux0[2][1] = 1                                                             # chain 1 holds half 1
    for series, start in ((far, h0), (zero, h0), (y, float("nan")), (y, float("inf"))):
        r = _run(th, ll0, L, prior, start, series, N, 4, 77, _clone(aux0))
        assert np.all(r["ll_prop"] == -np.inf) and not r["accept"].any()
        assert np.array_equal(_bits(r["theta_end"]), _bits(th)) and np.array_equal(r["ll_end"], ll0)
        assert np.array_equal(r["ll_chain"], np.repeat(ll0[:, None], 4, 1))
        assert r["aux_sel"].tolist() == [0, 1, 0]
        for c, half in enumerate((0, 1, 0)):                                   # the chain's own half is untouched
            assert np.array_equal(_bits(r["aux_n"][c, half]), _bits(aux0[0][c, half].cpu().numpy()))
            assert np.array_equal(_bits(r["aux_r"][c, half]), _bits(aux0[1][c, half].cpu().numpy()))
    r = _run(th, np.full(C, -np.inf), L, prior, h0, far, N, 2, 77, _clone(aux0))
    assert not r["accept"].any() and np.all(r["ll_end"] == -np.inf)           # -inf against -inf: NaN, rejected
    r = _run(th, np.full(C, -np.inf), L, prior, h0, y, N, 3, 77, _clone(aux0))
    assert np.isfinite(r["ll_prop"][:, 0]).all() and np.all(r["accept"][:, 0] == 1)
    assert np.array_equal(_bits(r["theta_chain"][:, 0]), _bits(r["theta_prop"][:, 0]))
    assert np.array_equal(r["ll_chain"][:, 0], r["ll_prop"][:, 0])


@pytest.mark.parametrize("N,T", [(64, 65), (1024, 5)])
def test_adaptation_replays_and_freezes(N, T):
    """adapt_end = 33 over the iterations 30 .. 34: chol_trace is tests/pmmh_adapt_ref.py's update of the factor before
    from the device's own xi, alpha and eta, bit for bit, and stands still from iteration 33 on; alpha is the numpy
    value of the recorded numbers within 1e-13; and the frozen iterations are the fixed chain (adapt_end = 0) started
    from the factor, the state and the aux the adapting launch left."""
    C, it0, end = 3, 30, 33
    th, y, prior, L = _setup(C, T, 3 + N)
    L[np.diag_indices(P)] = np.abs(np.diag(L))
    chol = np.stack([L * (1.0 + 0.5 * c) * 20.0 for c in range(C)]).astype(np.float32)
    h0, row0 = SR.FIX_H0, 999
    aux0 = _fresh(C, T, N)
    ll0 = _sorted_ll(th, h0, y, N, aux0[0][:, 0], aux0[1][:, 0])
    full = _run(th, ll0, chol, prior, h0, y, N, 5, row0, _clone(aux0), it0=it0, adapt_end=end)
    _, _, _, cur = MR.replay(th, ll0, prior, full["theta_prop"], full["ll_prop"], full["logu"])
    for c in range(C):
        Lc, ll, lp = np.tril(chol[c]).astype(np.float32), float(ll0[c]), MR.log_prior(th[c], prior)
        for i in range(5):
            lpp = MR.log_prior(full["theta_prop"][c, i], prior)
            al = AR.alpha(full["ll_prop"][c, i], ll, lpp, lp)
            assert abs(full["alpha_trace"][c, i] - al) <= 1e-13 * max(al, 1e-300)
            if it0 + i < end:
                assert abs(full["eta_trace"][c, i] - AR.eta(P, it0 + i, AR.GAMMA)) <= 1e-13
                Lc, _ = AR.adapt(Lc, full["xi_trace"][c, i][:P], full["alpha_trace"][c, i], full["eta_trace"][c, i],
                                 AR.TARGET)
            else:
                assert full["eta_trace"][c, i] == 0.0
            assert np.array_equal(_bits(full["chol_trace"][c, i]), _bits(Lc)), (c, i)
            if full["accept"][c, i]:
                ll, lp = float(full["ll_prop"][c, i]), lpp
    assert not np.array_equal(full["chol_trace"][:, 2], full["chol_trace"][:, 1])
    assert np.array_equal(_bits(full["chol_end"]), _bits(full["chol_trace"][:, -1]))
    aux = _clone(aux0)
    a = _run(th, ll0, chol, prior, h0, y, N, 3, row0, aux, it0=it0, adapt_end=end)
    b = _run(a["theta_end"], a["ll_end"], a["chol_end"], prior, h0, y, N, 2, row0, aux, it0=it0 + 3, adapt_end=0)
    for k in CHAIN:
        assert np.array_equal(_bits(b[k]), _bits(full[k][:, 3:])), k
    _same(b, full, ("theta_end", "ll_end", "chol_end", "aux_n", "aux_r", "aux_sel"))


def test_refusals_on_the_gpu():
    from viforssms_amd import ops
    C, N, T = 2, 64, 8
    th, y, prior, L = _setup(C, T, 1)
    aux = _fresh(C, T, N)
    ll = np.zeros(C)
    run = lambda a, **kw: _run(th, ll, L, prior, SR.FIX_H0, y, N, 1, 0, a, **kw)
    with pytest.raises(ValueError, match="aux_n"):
        run((aux[0][:, :1].contiguous(), aux[1], aux[2]))
    with pytest.raises(ValueError, match="aux_n"):
        run((aux[0].transpose(2, 3), aux[1], aux[2]))
    with pytest.raises(ValueError, match="aux_r"):
        run((aux[0], aux[1][:, :, :7].contiguous(), aux[2]))
    with pytest.raises(ValueError, match="aux_sel"):
        run((aux[0], aux[1], aux[2].long()))
    with pytest.raises(ValueError, match="aux_sel"):
        run((aux[0], aux[1], torch.full_like(aux[2], 2)))
    with pytest.raises(ValueError, match="rho"):
        run(aux, rho=1.0)
    r = _run(th, ll, L, prior, SR.FIX_H0, y, N, 0, 0, aux)                  # n_iter = 0: the state comes back
    assert r["theta_chain"].shape == (C, 0, P) and np.array_equal(_bits(r["theta_end"]), _bits(th))
    assert not r["aux_sel"].any()


# ----------------------------------------------------------------------------------------------------------------
# statistical
# ----------------------------------------------------------------------------------------------------------------
def _fixture_run(adapt_end):
    t = VR.truth("exact")
    y = VR.stat_series().astype(np.float32)
    C, N, n_iter = 64, 64, 1500
    th0 = VR.stat_start(t, C, 1)
    aux = _fresh(C, len(y) - 1, N, row0=0)
    ll0 = _sorted_ll(th0, SR.FIX_H0, y, N, aux[0][:, 0], aux[1][:, 0])
    r = _run(th0, ll0, t["L"], t["prior"], SR.FIX_H0, y, N, n_iter, C * N, aux, seed=SEED + 1, trace=False,
             adapt_end=adapt_end)
    assert np.isfinite(r["ll_chain"]).all()
    s = MR.summarise(r["theta_chain"][:, 300:].astype(np.float64), r["accept"][:, 300:])
    bars = MR.stat_bars(s, t)
    print({k: np.round(v, 4) for k, v in s.items()}, bars)
    return bars


def test_chains_meet_the_exact_posterior_acceptance_included():
    """The SV fixture (T = 64), C = 64 chains, N = 64 particles, rho = 0.99, 1500 iterations of which 300 are dropped,
    the fixture's L and a spread start: pmmh_ref.stat_bars against the exact (grid) chain's truth, its acceptance
    included -- the bar the ordinary kernel at N = 64 cannot meet (its own test compares with the numpy PMMH
    reference's acceptance at N = 64, 13 se lower), and which a chain without the sort or without the carried noise
    would miss the same way."""
    bars = _fixture_run(0)
    assert bars["ok"], bars


def test_adapted_chains_meet_the_exact_posterior():
    """The same with every chain adapting its factor over the first 300 iterations: the mean and sd bars only (the
    adapted chain aims at the target rate, not at the fixture's)."""
    bars = _fixture_run(300)
    assert (bars["dmean_over_se"] <= 4.0).all(), bars
    assert ((bars["sd_ratio"] >= 0.9) & (bars["sd_ratio"] <= 1.1)).all(), bars


# ----------------------------------------------------------------------------------------------------------------
# product
# ----------------------------------------------------------------------------------------------------------------
MC, MN, MITER, MBURN, T = 4, 64, 40, 10, 160
CPM_KEYS = MCMC_KEYS + ("mcmc/correlation",)


def _eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


@pytest.fixture(scope="module")
def sampled():
    from tests.parity_util import build_model
    model = build_model("sv", 7, 40, 8, 2, 16, 5, 3, DEV, T=T, precision=0, seed=3)
    return model, model.volatility_mcmc(MC, MN, MITER, MBURN, correlation=RHO)


def test_product_keys_shapes_and_by_hand_call(sampled):
    from viforssms_amd import diagnostics, ops
    model, got = sampled
    md = model.mdef
    assert sorted(got) == sorted(CPM_KEYS) and float(got["mcmc/correlation"]) == RHO
    assert got["mcmc/theta"].shape == (MC, MITER - MBURN, P) and got["mcmc/loglik"].shape == (MC, MITER - MBURN)
    assert got["mcmc/accept_rate"].shape == (MC,) and got["mcmc/rhat"].shape == (P,)
    _, theta = model.sample_paths_theta(np.tile(0, model.p_local), step=model.global_step)
    draw = theta.detach().float().contiguous()
    y = torch.as_tensor(np.asarray(model.obs, np.float32)[:T + 1], device=DEV)
    h0 = torch.full((1,), model.x0, device=DEV)
    seed = model.engine.seed ^ diagnostics.MCMC_SEED_XOR
    row0 = model.global_step * MC * MN * (MITER + 1)
    th = draw[:MC].contiguous()
    aux = ops.cpm_fresh_aux(MC, T, MN, seed ^ diagnostics.CPM_SEED_XOR, row0, DEV)
    ll = ops.sv_filter_sorted(th, h0, y, md.dt, MN, aux[0][:, 0].contiguous(), aux[1][:, 0].contiguous()).loglik
    chol = g(got["mcmc/prop_chol"].astype(np.float32)).repeat(MC, 1, 1)
    r = ops.sv_cpmmh(th, ll, chol, g(np.asarray(md.priors, np.float32)), h0, y, md.dt, MN, MITER, seed, row0 + MC * MN,
                     RHO, *aux)
    assert np.array_equal(_bits(got["mcmc/theta"]), _bits(r.theta_chain[:, MBURN:].cpu().numpy()))
    assert np.array_equal(_bits(got["mcmc/loglik"]), _bits(r.ll_chain[:, MBURN:].cpu().numpy()))
    assert np.isfinite(got["mcmc/loglik"]).any(), "every chain sits at -inf: nothing is compared"


def test_product_launch_cutting_zero_correlation_adapt_and_refusals(sampled, tmp_path, monkeypatch):
    from viforssms_amd import diagnostics, ops
    model, got = sampled
    calls = []
    real = ops.sv_cpmmh
    monkeypatch.setattr(ops, "sv_cpmmh", lambda *a, **kw: calls.append((a[8], kw.get("it0"))) or real(*a, **kw))
    monkeypatch.setattr(diagnostics, "MCMC_LAUNCH_STEPS", T * 7 + 3)          # seven iterations per launch
    path = str(tmp_path / "sub" / "cpm.npz")
    cut = model.save_volatility_mcmc(path, MC, MN, MITER, MBURN, correlation=RHO)
    assert calls == [(7, 0), (7, 7), (7, 14), (7, 21), (7, 28), (5, 35)]
    for k in CPM_KEYS:
        assert _eq(cut[k], got[k]), k
    with np.load(path) as z:
        assert sorted(z.files) == sorted(CPM_KEYS)
        for k in CPM_KEYS:
            assert _eq(z[k], got[k]), k
    # adapt composes: the two keys it adds, and the cut run is the uncut one
    cut_a = model.volatility_mcmc(MC, MN, MITER, MBURN, adapt=True, correlation=RHO)
    monkeypatch.setattr(diagnostics, "MCMC_LAUNCH_STEPS", 1 << 18)
    calls.clear()
    whole_a = model.volatility_mcmc(MC, MN, MITER, MBURN, adapt=True, correlation=RHO)
    assert calls == [(MITER, 0)]
    assert sorted(whole_a) == sorted(CPM_KEYS + ("mcmc/prop_chol_end", "mcmc/accept_rate_adapt"))
    for k in whole_a:
        assert _eq(cut_a[k], whole_a[k]), k
    # correlation = 0.0 is today's path, bit for bit, and never reaches the new entry
    calls.clear()
    plain, zero = model.volatility_mcmc(MC, MN, MITER, MBURN), model.volatility_mcmc(MC, MN, MITER, MBURN, correlation=0.0)
    assert not calls and sorted(zero) == sorted(MCMC_KEYS)
    for k in MCMC_KEYS:
        assert _eq(zero[k], plain[k]), k
    assert not _eq(got["mcmc/loglik"], plain["mcmc/loglik"])                  # (the correlated run is another chain)
    for rho in (-0.5, 1.0, 0.99999, float("nan")):
        with pytest.raises(ValueError, match="correlation"):
            model.volatility_mcmc(MC, MN, MITER, MBURN, correlation=rho)
    from tests.parity_util import filter_model
    with pytest.raises(ValueError, match="correlation"):
        filter_model("ar").theta_mcmc(4, 64, 10, 2, correlation=RHO)


def test_run_writes_the_chains(tmp_path, monkeypatch):
    """viforssms_amd.sv.run (SV_dense.py's driver) ... --mcmc 4 64 12 PATH --mcmc-adapt --mcmc-corr 0.99."""
    from viforssms_amd import sv
    state = np.random.get_state()
    monkeypatch.chdir(tmp_path)
    try:
        out = str(tmp_path / "post" / "cpm.npz")
        model = sv.run(["-p", "8", "--kernel-len", "8", "--batch-dims", "26", "--no-flows", "2", "--feat-window", "3",
                        "--steps", "2", "--no-pretrain", "--mcmc", "4", "64", "12", out, "--mcmc-adapt", "--mcmc-corr",
                        "0.99"])
    finally:
        np.random.set_state(state)
    assert model.global_step == 2
    with np.load(out) as z:
        assert sorted(z.files) == sorted(CPM_KEYS + ("mcmc/prop_chol_end", "mcmc/accept_rate_adapt"))
        assert z["mcmc/theta"].shape == (4, 6, P) and float(z["mcmc/correlation"]) == 0.99
