"""vissm_sv_pmmh (ops.sv_pmmh) on the GPU.

Replay: the traced proposals and log u are those of the host restatement (tests/svpmmh_ref.py) from the chain's
previous state; each proposal's estimate is ops.sv_filter(cloud=False) on the recorded proposals at row0 + i C N, bit
for bit; the decisions are the double rule applied to the recorded numbers, and the chain is their replay, bit for bit.
Chained, repeated, untraced and single-chain launches are compared bitwise; a series that kills every filter leaves the
chain where it was and a chain entering at -inf takes the first finite proposal; the chains' draws meet the grid
posterior of the SV fixture; the product path cuts its launches without changing a bit."""
import itertools
import os

import numpy as np
import pytest
import torch

from tests import pmmh_ref as MR
from tests import svf_ref as SR
from tests import svpmmh_ref as VR
from tests.sim_util import PF_SEED as SEED, bits as _bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, P = 1.0, VR.P
KEYS = ("theta_chain", "ll_chain", "accept", "theta_end", "ll_end", "theta_prop", "ll_prop", "logu")


def g(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _filter_ll(th, h0, y, N, row0, seed=SEED):
    from viforssms_amd import ops
    return ops.sv_filter(g(th), g(np.array([h0], np.float32)), g(y), DT, N, seed, row0, cloud=False).loglik.cpu().numpy()


def _run(th, ll, L, prior, h0, y, N, n_iter, row0, it0=0, trace=True, seed=SEED):
    from viforssms_amd import ops
    r = ops.sv_pmmh(g(th), g(np.asarray(ll, np.float64)), g(L), g(prior), g(np.array([h0], np.float32)), g(y), DT, N,
                    n_iter, seed, row0, it0=it0, trace=trace)
    torch.cuda.synchronize()
    return {k: (None if getattr(r, k) is None else getattr(r, k).cpu().numpy()) for k in KEYS}


def _same(a, b, keys=KEYS):
    for k in keys:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def _setup(C, T, seed):
    """theta within 0.1 of PARAM_INIT with |theta_0| in [0.01, 0.1], a series simulated at PARAM_INIT, a prior two
    units wide around theta, and a factor whose rows p >= 1 sum to at most 0.01 in absolute value and whose row 0 is
    scaled by min |theta_0| / 0.45 (see test_replay)."""
    rng = np.random.default_rng(seed)
    th = (np.asarray(SR.PARAM_INIT) + rng.uniform(-0.1, 0.1, (C, P))).astype(np.float32)
    th[:, 0] = (rng.choice([-1.0, 1.0], C) * rng.uniform(0.01, 0.1, C)).astype(np.float32)
    y, _ = SR.simulate_series(T, SR.PARAM_INIT, DT, SR.FIX_H0, 1.0, rng)
    prior = np.stack([np.asarray(SR.PARAM_INIT) + 0.3, np.full(P, 2.0)], 1).astype(np.float32)
    L = 0.002 * np.tril(rng.choice([-1.0, 1.0], (P, P)) * rng.uniform(0.5, 1.0, (P, P)))
    L[0] *= float(np.abs(th[:, 0]).min()) / 0.45
    return th, y, prior, L.astype(np.float32)


def _ulps32(a, b):
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b).astype(np.float32))


REPLAY = list(itertools.product((64, 128, 1024), (1, 3), (1, 5), (1, 4, 5, 63, 65)))
# four and eight waves: two and four trips of the partial-sum loop
REPLAY += list(itertools.product((256, 512), (1, 3), (1, 5), (5, 65)))


@pytest.mark.parametrize("N,C,n_iter,T", REPLAY)
def test_replay(N, C, n_iter, T):
    """T = 1 is one step, 4 and 5 sit on the Philox group boundary of the one-normal stream, 63 and 65 are more than
    one group with an odd tail.  theta_prop within 1 ulp fp32 (tests/test_gpu_pmmh.py's bar) and log u within 2 ulp of
    the host restatement made from the chain's previous state: the device's normals come from the hardware
    transcendentals and the restatement's from float64, about 1e-6 apart, which a factor whose row sums to 0.01
    |theta_p| / 0.45 turns into under half an ulp of theta_p -- the rounded sums differ by at most one ulp, and cannot
    be promised equal (measured on one MI355X: 4 of the 1440 elements of the 60 cases are one ulp off; the count of
    equal ones is printed).  ll_prop is ops.sv_filter's loglik on the recorded proposals, bit for bit; accept,
    theta_chain and ll_chain are the replay of the double rule over the recorded numbers, bit for bit."""
    from viforssms_amd import ops
    th, y, prior, L = _setup(C, T, 1000 * N + 100 * C + 10 * n_iter + T)
    h0, row0 = SR.FIX_H0, 11 + 5 * N
    ll0 = _filter_ll(th, h0, y, N, row0)
    base = row0 + C * N
    r = _run(th, ll0, L, prior, h0, y, N, n_iter, base)
    assert r["theta_prop"].shape == (C, n_iter, P) and r["ll_prop"].shape == (C, n_iter) and r["accept"].dtype == np.int32
    th_chain, ll_chain, acc, cur = MR.replay(th, ll0, prior, r["theta_prop"], r["ll_prop"], r["logu"])
    worst_t = worst_u = 0.0
    equal = 0
    for c in range(C):
        for i in range(n_iter):
            _, want, _, lu = VR.iteration(SEED, base, i, C, c, N, cur[c, i], L, prior)
            worst_t = max(worst_t, float(_ulps32(r["theta_prop"][c, i], want).max()))
            equal += int((_bits(r["theta_prop"][c, i]) == _bits(want)).sum())
            worst_u = max(worst_u, abs(r["logu"][c, i] - lu) / np.spacing(abs(lu)))
    h0_d, y_d = g(np.array([h0], np.float32)), g(y)
    ll_want = np.stack([ops.sv_filter(g(r["theta_prop"][:, i]), h0_d, y_d, DT, N, SEED, base + i * C * N,
                                      cloud=False).loglik.cpu().numpy() for i in range(n_iter)], 1)
    print(f"N {N} C {C} n_iter {n_iter} T {T}: theta_prop {worst_t:.2f} ulp ({equal} of {C * n_iter * P} equal), logu "
          f"{worst_u:.2f} ulp, |ll_prop - filter| {np.max(np.abs(r['ll_prop'] - ll_want)):.3e}, accepted "
          f"{int(r['accept'].sum())} of {C * n_iter}")
    assert worst_t <= 1.0 and worst_u <= 2.0
    assert np.isfinite(r["ll_prop"]).all() and np.isfinite(ll_want).all(), "the stable-range inputs left the domain"
    assert np.array_equal(_bits(r["ll_prop"]), _bits(ll_want))
    assert np.array_equal(r["accept"], acc)
    assert np.array_equal(_bits(r["theta_chain"]), _bits(th_chain))
    assert np.array_equal(_bits(r["ll_chain"]), _bits(ll_chain))
    assert np.array_equal(_bits(r["theta_end"]), _bits(th_chain[:, -1]))
    assert np.array_equal(_bits(r["ll_end"]), _bits(ll_chain[:, -1]))


@pytest.mark.parametrize("N,T", [(64, 65), (1024, 63), (128, 5)])
def test_chaining_repeat_and_independence_of_the_block(N, T):
    """3 + 2 iterations chained through theta_end / ll_end are the five of one launch; two launches agree; without
    the traces the outputs are the same; and chain 2 of three, whose iteration i sits on row r = row0 + (3 i + 2) N,
    is reproduced by single-chain launches of one iteration placed on that row."""
    C = 3
    th, y, prior, L = _setup(C, T, 7 + N)
    L = (L * 20.0).astype(np.float32)               # steps wide enough for both decisions to occur
    h0, row0 = SR.FIX_H0, 12345
    ll0 = _filter_ll(th, h0, y, N, 99)
    full = _run(th, ll0, L, prior, h0, y, N, 5, row0)
    _same(full, _run(th, ll0, L, prior, h0, y, N, 5, row0))
    plain = _run(th, ll0, L, prior, h0, y, N, 5, row0, trace=False)
    assert plain["theta_prop"] is None and plain["ll_prop"] is None and plain["logu"] is None
    _same(full, plain, KEYS[:5])
    a = _run(th, ll0, L, prior, h0, y, N, 3, row0)
    b = _run(a["theta_end"], a["ll_end"], L, prior, h0, y, N, 2, row0, it0=3)
    for k in ("theta_chain", "ll_chain", "accept", "theta_prop", "ll_prop", "logu"):
        assert np.array_equal(_bits(np.concatenate([a[k], b[k]], 1)), _bits(full[k])), k
    _same(b, full, ("theta_end", "ll_end"))
    c, t, ll = 2, th[2:3], ll0[2:3]
    for i in range(5):
        # a single chain at it0 = i sits on row0' + i N: place it on row0 + (3 i + 2) N
        one = _run(t, ll, L, prior, h0, y, N, 1, row0 + (3 * i + c) * N - i * N, it0=i)
        for k in ("theta_chain", "ll_chain", "accept", "theta_prop", "ll_prop", "logu"):
            assert np.array_equal(_bits(one[k][0, 0]), _bits(full[k][c, i])), (k, i)
        t, ll = one["theta_end"], one["ll_end"]


def test_dead_proposals_and_a_chain_entering_at_minus_infinity():
    """A value 1e30 away in y (the squared residual overflows fp32, so no particle has a finite weight), a zero inside
    y (the next step's weights are NaN) and a start that is not finite kill every filter: ll_prop = -inf, nothing is
    accepted and the chain stays where it was, ll included.  A chain entering at ll = -inf (with ordinary data) takes
    its first finite proposal, whatever log u is."""
    C, N, T = 3, 128, 20
    th, y, prior, L = _setup(C, T, 5)
    h0 = SR.FIX_H0
    far, zero = y.copy(), y.copy()
    far[7], zero[9] = 1e30, 0.0
    ll0 = np.array([-5.0, -6.0, -7.0])
    for series, start in ((far, h0), (zero, h0), (y, float("nan")), (y, float("inf"))):
        r = _run(th, ll0, L, prior, start, series, N, 4, 77)
        assert np.all(r["ll_prop"] == -np.inf) and not r["accept"].any()
        assert np.array_equal(_bits(r["theta_chain"]), _bits(np.repeat(th[:, None, :], 4, 1)))
        assert np.array_equal(r["ll_chain"], np.repeat(ll0[:, None], 4, 1))
        assert np.array_equal(_bits(r["theta_end"]), _bits(th)) and np.array_equal(r["ll_end"], ll0)
        assert np.all(_filter_ll(th, start, series, N, 77) == -np.inf)      # the filter entry agrees
    # -inf against -inf: NaN, rejected, and the chain's -inf stays
    r = _run(th, np.full(C, -np.inf), L, prior, h0, far, N, 2, 77)
    assert not r["accept"].any() and np.all(r["ll_end"] == -np.inf)
    r = _run(th, np.full(C, -np.inf), L, prior, h0, y, N, 3, 77)
    assert np.isfinite(r["ll_prop"][:, 0]).all() and np.all(r["accept"][:, 0] == 1)
    assert np.array_equal(_bits(r["theta_chain"][:, 0]), _bits(r["theta_prop"][:, 0]))
    assert np.array_equal(r["ll_chain"][:, 0], r["ll_prop"][:, 0])
    # T = 0: nothing to filter, ll' = 0
    r = _run(th, ll0, L, prior, h0, y[:1], N, 2, 77)
    assert np.all(r["ll_prop"] == 0.0) and r["accept"].all()


def test_refusals_on_the_gpu():
    from viforssms_amd import ops
    th, y, prior, L = _setup(2, 8, 1)
    ll, h0 = np.zeros(2), np.array([SR.FIX_H0], np.float32)
    with pytest.raises(ValueError, match="ll_cur"):
        ops.sv_pmmh(g(th), g(ll.astype(np.float32)), g(L), g(prior), g(h0), g(y), 1.0, 64, 1, 1, 0)
    with pytest.raises(ValueError, match="ll_cur"):
        ops.sv_pmmh(g(th), g(np.zeros(3)), g(L), g(prior), g(h0), g(y), 1.0, 64, 1, 1, 0)
    with pytest.raises(ValueError, match="prop_chol"):
        ops.sv_pmmh(g(th), g(ll), g(L[:2]), g(prior), g(h0), g(y), 1.0, 64, 1, 1, 0)
    with pytest.raises(ValueError, match="prior"):
        ops.sv_pmmh(g(th), g(ll), g(L), g(prior[:3]), g(h0), g(y), 1.0, 64, 1, 1, 0)
    with pytest.raises(ValueError, match="h_start"):
        ops.sv_pmmh(g(th), g(ll), g(L), g(prior), g(np.zeros(2, np.float32)), g(y), 1.0, 64, 1, 1, 0)
    with pytest.raises(ValueError, match="obs"):
        ops.sv_pmmh(g(th), g(ll), g(L), g(prior), g(h0), g(y[None, :]), 1.0, 64, 1, 1, 0)
    with pytest.raises(ValueError, match="obs"):
        ops.sv_pmmh(g(th), g(ll), g(L), g(prior), g(h0), g(y.astype(np.float64)), 1.0, 64, 1, 1, 0)
    r = _run(th, ll, L, prior, SR.FIX_H0, y, 64, 0, 0)                    # n_iter = 0: the state comes back
    assert r["theta_chain"].shape == (2, 0, P) and np.array_equal(_bits(r["theta_end"]), _bits(th))


# ----------------------------------------------------------------------------------------------------------------
# statistical
# ----------------------------------------------------------------------------------------------------------------
def test_chains_meet_the_grid_posterior():
    """The SV fixture (T = 64, dt = 1, h_0 = -8.5, prior N(PARAM_INIT, (0.05, 0.2, 0.3, 0.3)^2)), C = 64 chains, N = 64
    particles, 1500 iterations of which 300 are dropped, with the fixture's L and a spread start.  Mean and sd against
    the exact (grid) chain's truth -- PMMH is exact for any N -- and the acceptance against the numpy PMMH reference's
    at the same N = 64, because the estimate's noise lowers the acceptance itself: |mean - truth| <= 4 sqrt(se^2 +
    se_truth^2) per coordinate, pooled sd ratio in [0.9, 1.1], |acceptance - the reference's| <= 4 se between chains."""
    t = VR.truth("ref64")
    y = VR.stat_series().astype(np.float32)
    C, N, n_iter, burn = 64, 64, 1500, 300
    th0 = VR.stat_start(t, C, 1)
    ll0 = _filter_ll(th0, SR.FIX_H0, y, N, 0, seed=SEED + 1)
    r = _run(th0, ll0, t["L"], t["prior"], SR.FIX_H0, y, N, n_iter, C * N, seed=SEED + 1, trace=False)
    s = MR.summarise(r["theta_chain"][:, burn:].astype(np.float64), r["accept"][:, burn:])
    bars = MR.stat_bars(s, t)
    print({k: np.round(v, 4) for k, v in s.items()}, bars)
    assert np.isfinite(r["ll_chain"]).all()
    assert bars["ok"], bars


# ----------------------------------------------------------------------------------------------------------------
# product
# ----------------------------------------------------------------------------------------------------------------
MC, MN, MITER, MBURN, T = 4, 64, 40, 10, 160
MCMC_KEYS = ("probs", "mcmc/theta", "mcmc/loglik", "mcmc/accept_rate", "mcmc/prop_chol", "mcmc/mean", "mcmc/sd",
             "mcmc/quantiles", "mcmc/rhat", "theta/mean", "theta/sd", "theta/quantiles")


def _eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


@pytest.fixture(scope="module")
def sampled():
    from tests.parity_util import build_model
    model = build_model("sv", 7, 40, 8, 2, 16, 5, 3, DEV, T=T, precision=0, seed=3)
    return model, model.volatility_mcmc(MC, MN, MITER, MBURN)


def test_product_keys_shapes_and_by_hand_call(sampled):
    from viforssms_amd import diagnostics, ops
    model, got = sampled
    md = model.mdef
    assert sorted(got) == sorted(MCMC_KEYS)
    shapes = {"probs": (5,), "mcmc/theta": (MC, MITER - MBURN, P), "mcmc/loglik": (MC, MITER - MBURN),
              "mcmc/accept_rate": (MC,), "mcmc/prop_chol": (P, P), "mcmc/mean": (P,), "mcmc/sd": (P,),
              "mcmc/quantiles": (5, P), "mcmc/rhat": (P,), "theta/mean": (P,), "theta/sd": (P,),
              "theta/quantiles": (5, P)}
    for k, shp in shapes.items():
        assert got[k].shape == shp, k
    _, theta = model.sample_paths_theta(np.tile(0, model.p_local), step=model.global_step)
    draw = theta.detach().float().contiguous()
    chol = np.linalg.cholesky(2.38 ** 2 / P * np.cov(draw.cpu().numpy().astype(np.float64).T))
    assert np.array_equal(got["mcmc/prop_chol"], chol)
    summary = model.posterior_summary()
    for k in ("mean", "sd", "quantiles"):
        assert np.array_equal(got[f"theta/{k}"], summary[f"theta/{k}"]), k
    y = torch.as_tensor(np.asarray(model.obs, np.float32)[:T + 1], device=DEV)
    h0 = torch.full((1,), model.x0, device=DEV)
    seed = model.engine.seed ^ diagnostics.MCMC_SEED_XOR
    row0 = model.global_step * MC * MN * (MITER + 1)
    th = draw[:MC].contiguous()
    ll = ops.sv_filter(th, h0, y, md.dt, MN, seed, row0, cloud=False).loglik
    r = ops.sv_pmmh(th, ll, g(chol.astype(np.float32)), g(np.asarray(md.priors, np.float32)), h0, y, md.dt, MN, MITER,
                    seed, row0 + MC * MN)
    assert np.array_equal(_bits(got["mcmc/theta"]), _bits(r.theta_chain[:, MBURN:].cpu().numpy()))
    assert np.array_equal(_bits(got["mcmc/loglik"]), _bits(r.ll_chain[:, MBURN:].cpu().numpy()))
    assert np.array_equal(got["mcmc/accept_rate"], r.accept[:, MBURN:].double().mean(1).cpu().numpy())
    assert np.isfinite(got["mcmc/loglik"]).any(), "every chain sits at -inf: nothing is compared"
    pooled = got["mcmc/theta"].reshape(-1, P).astype(np.float64)
    pooled[:, 2:] = np.exp(pooled[:, 2:])                                   # theta_pos of SV
    assert np.allclose(got["mcmc/mean"], pooled.mean(0), rtol=1e-5)
    assert np.allclose(got["mcmc/quantiles"], np.quantile(pooled, got["probs"], axis=0), rtol=1e-5)


def test_product_launch_cutting_save_and_refusals(sampled, tmp_path, monkeypatch):
    from tests.parity_util import filter_model
    from viforssms_amd import diagnostics, ops
    model, got = sampled
    calls = []
    real = ops.sv_pmmh
    monkeypatch.setattr(ops, "sv_pmmh", lambda *a, **kw: calls.append((a[8], kw.get("it0"))) or real(*a, **kw))
    monkeypatch.setattr(diagnostics, "MCMC_LAUNCH_STEPS", T * 7 + 3)          # seven iterations per launch
    path = str(tmp_path / "sub" / "mcmc.npz")
    cut = model.save_volatility_mcmc(path, MC, MN, MITER, MBURN)
    assert calls == [(7, 0), (7, 7), (7, 14), (7, 21), (7, 28), (5, 35)]
    for k in MCMC_KEYS:
        assert _eq(cut[k], got[k]), k
    with np.load(path) as z:
        assert sorted(z.files) == sorted(MCMC_KEYS)
        for k in MCMC_KEYS:
            assert _eq(z[k], got[k]), k
    monkeypatch.setattr(diagnostics, "MCMC_LAUNCH_STEPS", 1)                  # at least one iteration per launch
    calls.clear()
    one = model.volatility_mcmc(MC, MN, 4, 1)
    assert calls == [(1, i) for i in range(4)] and one["mcmc/theta"].shape == (MC, 3, P)
    base = dict(n_chains=MC, n_particles=MN, n_iter=MITER, burn_in=MBURN)
    for kw, msg in ((dict(n_particles=96), "n_particles"), (dict(n_chains=0), "n_chains"),
                    (dict(n_chains=model.p_local + 1), "n_chains"), (dict(n_iter=5, burn_in=5), "burn_in"),
                    (dict(step_scale=0.0), "step_scale"), (dict(step_scale=float("inf")), "step_scale")):
        with pytest.raises(ValueError, match=msg):
            model.volatility_mcmc(**{**base, **kw})
    keep = model.obs
    try:
        for t, v, what in ((17, 0.0, "= 0"), (T - 1, 0.0, "= 0"), (5, np.nan, "finite"), (T, np.inf, "finite")):
            model.obs = keep.copy()
            model.obs[t] = v
            with pytest.raises(ValueError, match=what):
                model.volatility_mcmc(**base)
    finally:
        model.obs = keep
    with pytest.raises(ValueError, match="SV"):                              # the existing entry still refuses SV
        model.theta_mcmc(MC, MN, 10, 2)
    with pytest.raises(ValueError, match="theta_mcmc"):
        filter_model("ar").volatility_mcmc(4, 64, 10, 2)


def test_run_writes_the_chains(tmp_path, monkeypatch):
    """viforssms_amd.sv.run (SV_dense.py's driver) ... --mcmc 4 64 12 PATH: two training steps, then the .npz."""
    from viforssms_amd import sv
    state = np.random.get_state()
    monkeypatch.chdir(tmp_path)
    try:
        out = str(tmp_path / "post" / "mcmc.npz")
        model = sv.run(["-p", "8", "--kernel-len", "8", "--batch-dims", "26", "--no-flows", "2", "--feat-window", "3",
                        "--steps", "2", "--no-pretrain", "--mcmc", "4", "64", "12", out])
    finally:
        np.random.set_state(state)
    assert model.global_step == 2
    with np.load(out) as z:
        assert sorted(z.files) == sorted(MCMC_KEYS)
        assert z["mcmc/theta"].shape == (4, 9, P) and z["mcmc/quantiles"].shape == (5, P) and z["mcmc/rhat"].shape == (P,)
