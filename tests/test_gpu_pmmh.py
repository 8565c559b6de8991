"""vissm_pmmh (ops.pmmh) on the GPU.

Replay: the traced proposals and log u are those of the host restatement (tests/pmmh_ref.py) from the chain's previous
state; each proposal's estimate is ops.particle_filter(proposal="adapted", cloud=False) on the recorded proposals at
row0 + i C N; the decisions are the double rule applied to the recorded numbers, and the chain is their replay, bit for
bit.  Chained, repeated and single-chain launches are compared bitwise; a proposal that always dies leaves the chain
where it was and a chain entering at -inf takes the first finite proposal; the chains' draws meet the exact posterior
of the AR fixture under both priors; the product path cuts its launches without changing a bit."""
import os

import numpy as np
import pytest
import torch

from tests import pf_ref as PR
from tests import pmmh_ref as MR
from tests import sim_util as SU
from tests.parity_util import filter_model
from tests.sim_util import PF_OBS_STD as OBS_STD, PF_SEED as SEED, bits as _bits, filter_series as _series

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("theta_chain", "ll_chain", "accept", "theta_end", "ll_end", "theta_prop", "ll_prop", "logu")


def g(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _filter(model, th, x0, obs, obs_bin, N, row0, obs_std=None, seed=SEED):
    """(loglik [K], ll_inc [K, T]) of the adapted filter without its cloud."""
    from viforssms_amd import ops
    r = ops.particle_filter(model, g(th), g(x0), g(obs), g(obs_bin), SU.DT[model],
                            OBS_STD[model] if obs_std is None else obs_std, N, seed, row0, cloud=False,
                            proposal="adapted")
    return r.loglik.cpu().numpy(), r.ll_inc.cpu().numpy()


def _filter_ll(*a, **kw):
    return _filter(*a, **kw)[0]


def _run(model, th, ll, L, prior, x0, obs, obs_bin, N, n_iter, row0, it0=0, trace=True, obs_std=None, seed=SEED):
    from viforssms_amd import ops
    r = ops.pmmh(model, g(th), g(np.asarray(ll, np.float64)), g(L), g(prior), g(x0), g(obs), g(obs_bin), SU.DT[model],
                 OBS_STD[model] if obs_std is None else obs_std, N, n_iter, seed, row0, it0=it0, trace=trace)
    torch.cuda.synchronize()
    return {k: (None if getattr(r, k) is None else getattr(r, k).cpu().numpy()) for k in KEYS}


def _same(a, b, keys=KEYS):
    for k in keys:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def _setup(model, C, T, pattern, seed):
    """theta within 10 % of the generator's (|theta_p| >= 0.45), a prior two units wide around it, and a factor whose
    rows sum to at most 0.01 in absolute value (see test_replay)."""
    rng = np.random.default_rng(seed)
    th, _ = SU.filter_inputs(model, C, 64, rng)
    P = SU.P_OF[model]
    x0 = np.asarray(SU.TRUE_X[model], np.float32)
    obs, obs_bin = _series(model, T, pattern, rng)
    prior = np.stack([np.asarray(SU.TRUE_THETA[model]) + 0.3, np.full(P, 2.0)], 1).astype(np.float32)
    L = (0.002 * np.tril(rng.choice([-1.0, 1.0], (P, P)) * rng.uniform(0.5, 1.0, (P, P)))).astype(np.float32)
    return th, x0, obs, obs_bin, prior, L


def _ulps32(a, b):
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b).astype(np.float32))


REPLAY = [(SU.AR, 3, 64, 65, 5, "all"), (SU.AR, 1, 1024, 63, 5, "tenth"), (SU.AR, 3, 128, 1, 1, "all"),
          (SU.LV, 3, 128, 65, 5, "all"), (SU.LV, 1, 64, 63, 5, "coord"), (SU.LV, 3, 1024, 65, 1, "tenth"),
          (SU.LV, 1, 128, 1, 5, "tenth"), (SU.FHN, 3, 64, 63, 5, "all"), (SU.FHN, 1, 1024, 65, 5, "coord"),
          (SU.FHN, 3, 128, 63, 1, "tenth"), (SU.FHN, 3, 1024, 1, 5, "all"),
          # four and eight waves: two and four trips of the partial-sum loop
          (SU.AR, 3, 256, 65, 5, "tenth"), (SU.LV, 3, 512, 65, 5, "coord"), (SU.FHN, 3, 256, 65, 5, "coord")]


@pytest.mark.parametrize("model,C,N,T,n_iter,pattern", REPLAY)
def test_replay(model, C, N, T, n_iter, pattern):
    """theta_prop within 1 ulp fp32 and log u within 2 ulp of the host restatement made from the chain's previous
    state.  The device's normals come from the hardware transcendentals (box_muller4) and the restatement's from
    float64: they differ by at most about 1e-6 in absolute value, which a factor whose rows sum to 0.01 turns into
    1e-8, under half an ulp of a theta of magnitude 0.45 or more (1.5e-8) -- so the rounded sums differ by at most
    one ulp.  ll_prop is the adapted filter's loglik on the recorded proposals: bit for bit for AR and FHN.  For LV
    the two kernels' fp32 weights contract differently (the same header inlined into two loops; measured: up to 7e-7
    on a loglik of -352 over 65 observed steps, every ancestor unchanged), so there ll_prop is held to
    tests/test_gpu_adapted.py's ll_inc bar summed over the observed steps -- its floor 8 * 2^-20 |ll_inc_t|, the
    smaller of that bar's two terms, from the filter's own increments (2.7e-3 in that case).  accept, theta_chain
    and ll_chain are the replay of the double rule over the recorded numbers, bit for bit."""
    th, x0, obs, obs_bin, prior, L = _setup(model, C, T, pattern, 100 * model + N + T + C)
    row0 = 11 + 5 * N
    ll0 = _filter_ll(model, th, x0, obs, obs_bin, N, row0)
    base = row0 + C * N
    r = _run(model, th, ll0, L, prior, x0, obs, obs_bin, N, n_iter, base)
    P = SU.P_OF[model]
    assert r["theta_prop"].shape == (C, n_iter, P) and r["ll_prop"].shape == (C, n_iter) and r["accept"].dtype == np.int32
    th_chain, ll_chain, acc, cur = MR.replay(th, ll0, prior, r["theta_prop"], r["ll_prop"], r["logu"])
    worst_t = worst_u = 0.0
    for c in range(C):
        for i in range(n_iter):
            row = MR.row_of(base, i, C, c, N)
            want = MR.propose(cur[c, i], L, MR.xi(SEED, row)[:P])
            worst_t = max(worst_t, float(_ulps32(r["theta_prop"][c, i], want).max()))
            lu = MR.log_u(SEED, row)
            worst_u = max(worst_u, abs(r["logu"][c, i] - lu) / np.spacing(abs(lu)))
    parts = [_filter(model, r["theta_prop"][:, i], x0, obs, obs_bin, N, base + i * C * N) for i in range(n_iter)]
    ll_want = np.stack([p[0] for p in parts], 1)
    ll_bar = np.stack([8.0 * 2.0 ** -20 * np.abs(p[1]).sum(1) for p in parts], 1)
    n_obs = int(np.any(obs_bin != 0, axis=0).sum())
    with np.errstate(invalid="ignore"):
        dll = np.nanmax(np.abs(np.where(np.isfinite(ll_want), r["ll_prop"] - ll_want, 0.0)))
    print(f"model {model} C {C} N {N} T {T} n_iter {n_iter} {pattern}: theta_prop {worst_t:.2f} ulp, logu "
          f"{worst_u:.2f} ulp, |ll_prop - filter| {dll:.3e} over {n_obs} observed steps, accepted "
          f"{int(r['accept'].sum())} of {C * n_iter}")
    assert worst_t <= 1.0 and worst_u <= 2.0
    assert np.isfinite(r["ll_prop"]).all() and np.isfinite(ll_want).all(), "the stable-range inputs left the domain"
    if model == SU.LV:
        assert np.all(np.abs(r["ll_prop"] - ll_want) <= ll_bar), float(np.max(np.abs(r["ll_prop"] - ll_want) / ll_bar))
    else:
        assert np.array_equal(_bits(r["ll_prop"]), _bits(ll_want))
    assert np.array_equal(r["accept"], acc)
    assert np.array_equal(_bits(r["theta_chain"]), _bits(th_chain))
    assert np.array_equal(_bits(r["ll_chain"]), _bits(ll_chain))
    assert np.array_equal(_bits(r["theta_end"]), _bits(th_chain[:, -1]))
    assert np.array_equal(_bits(r["ll_end"]), _bits(ll_chain[:, -1]))


@pytest.mark.parametrize("model,N,T", [(SU.AR, 64, 65), (SU.LV, 1024, 63), (SU.FHN, 128, 65)])
def test_chaining_repeat_and_independence_of_the_block(model, N, T):
    """3 + 2 iterations chained through theta_end / ll_end are the five of one launch; two launches agree; without
    the traces the outputs are the same; and chain 2 of three, whose iteration i sits on row r = row0 + (3 i + 2) N,
    is reproduced by single-chain launches of one iteration placed on that row: its bits depend on the block index
    and on C through r only."""
    C = 3
    th, x0, obs, obs_bin, prior, L = _setup(model, C, T, "all", 7 + model)
    row0 = 12345
    ll0 = _filter_ll(model, th, x0, obs, obs_bin, N, 99)
    full = _run(model, th, ll0, L, prior, x0, obs, obs_bin, N, 5, row0)
    _same(full, _run(model, th, ll0, L, prior, x0, obs, obs_bin, N, 5, row0))
    plain = _run(model, th, ll0, L, prior, x0, obs, obs_bin, N, 5, row0, trace=False)
    assert plain["theta_prop"] is None and plain["ll_prop"] is None and plain["logu"] is None
    _same(full, plain, KEYS[:5])
    a = _run(model, th, ll0, L, prior, x0, obs, obs_bin, N, 3, row0)
    b = _run(model, a["theta_end"], a["ll_end"], L, prior, x0, obs, obs_bin, N, 2, row0, it0=3)
    for k in ("theta_chain", "ll_chain", "accept", "theta_prop", "ll_prop", "logu"):
        assert np.array_equal(_bits(np.concatenate([a[k], b[k]], 1)), _bits(full[k])), k
    _same(b, full, ("theta_end", "ll_end"))
    c, t, ll = 2, th[2:3], ll0[2:3]
    for i in range(5):
        # a single chain at it0 = i sits on row0' + i N: place it on row0 + (3 i + 2) N
        one = _run(model, t, ll, L, prior, x0, obs, obs_bin, N, 1, row0 + (3 * i + c) * N - i * N, it0=i)
        for k in ("theta_chain", "ll_chain", "accept", "theta_prop", "ll_prop", "logu"):
            assert np.array_equal(_bits(one[k][0, 0]), _bits(full[k][c, i])), (k, i)
        t, ll = one["theta_end"], one["ll_end"]


def test_dead_proposals_and_a_chain_entering_at_minus_infinity():
    """An observation 1e30 away under obs_std = 1e-3 kills every filter (the squared residual overflows fp32, so no
    particle has a finite weight): ll_prop = -inf, nothing is accepted and the chain stays where it was, ll included.
    A chain entering at ll = -inf (with ordinary data) takes its first finite proposal, whatever log u is."""
    model, C, N, T = SU.AR, 3, 128, 20
    th, x0, obs, obs_bin, prior, L = _setup(model, C, T, "all", 5)
    far = obs.copy()
    far[:, 7] = 1e30
    ll0 = np.array([-5.0, -6.0, -7.0])
    r = _run(model, th, ll0, L, prior, x0, far, obs_bin, N, 4, 77, obs_std=1e-3)
    assert np.all(r["ll_prop"] == -np.inf) and not r["accept"].any()
    assert np.array_equal(_bits(r["theta_chain"]), _bits(np.repeat(th[:, None, :], 4, 1)))
    assert np.array_equal(r["ll_chain"], np.repeat(ll0[:, None], 4, 1))
    assert np.array_equal(_bits(r["theta_end"]), _bits(th)) and np.array_equal(r["ll_end"], ll0)
    # -inf against -inf: NaN, rejected, and the chain's -inf stays
    r = _run(model, th, np.full(C, -np.inf), L, prior, x0, far, obs_bin, N, 2, 77, obs_std=1e-3)
    assert not r["accept"].any() and np.all(r["ll_end"] == -np.inf)
    r = _run(model, th, np.full(C, -np.inf), L, prior, x0, obs, obs_bin, N, 3, 77)
    assert np.isfinite(r["ll_prop"][:, 0]).all() and np.all(r["accept"][:, 0] == 1)
    assert np.array_equal(_bits(r["theta_chain"][:, 0]), _bits(r["theta_prop"][:, 0]))
    assert np.array_equal(r["ll_chain"][:, 0], r["ll_prop"][:, 0])


def test_refusals_on_the_gpu():
    from viforssms_amd import ops
    th, x0, obs, obs_bin, prior, L = _setup(SU.AR, 2, 8, "all", 1)
    ll = np.zeros(2)
    with pytest.raises(ValueError, match="ll_cur"):
        ops.pmmh(SU.AR, g(th), g(ll.astype(np.float32)), g(L), g(prior), g(x0), g(obs), g(obs_bin), 1.0, 1.0, 64, 1, 1, 0)
    with pytest.raises(ValueError, match="prop_chol"):
        ops.pmmh(SU.AR, g(th), g(ll), g(L[:2]), g(prior), g(x0), g(obs), g(obs_bin), 1.0, 1.0, 64, 1, 1, 0)
    with pytest.raises(ValueError, match="x_start"):
        ops.pmmh(SU.AR, g(th), g(ll), g(L), g(prior), g(np.zeros((2, 1), np.float32)), g(obs), g(obs_bin), 1.0, 1.0,
                 64, 1, 1, 0)
    r = _run(SU.AR, th, ll, L, prior, x0, obs, obs_bin, 64, 0, 0)         # n_iter = 0: the state comes back
    assert r["theta_chain"].shape == (2, 0, 3) and np.array_equal(_bits(r["theta_end"]), _bits(th))


# ----------------------------------------------------------------------------------------------------------------
# statistical
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MR.PRIOR_CASES)
def test_chains_meet_the_exact_posterior(case):
    """AR fixture, C = 64 chains, N = 64 particles, 1500 iterations of which 300 are dropped, with the fixture's L,
    against the exact chain's truth: |mean - truth| <= 4 sqrt(se^2 + se_truth^2) per coordinate, pooled sd ratio in
    [0.9, 1.1], |acceptance - the truth's| <= 4 se between chains.  Under the informative prior on theta_0 a chain
    that dropped the prior would sit near the flat case's 7.67 instead of 5.24."""
    obs, obs_bin = PR.stat_case()
    t = MR.truth(case)
    C, N, n_iter, burn = 64, 64, 1500, 300
    th0 = MR.stat_start(t, C, 1)
    x0 = np.array([MR.STAT_X0], np.float32)
    ll0 = _filter_ll(SU.AR, th0, x0, obs, obs_bin, N, 0, obs_std=MR.STAT_OBS_STD, seed=SEED + 1)
    r = _run(SU.AR, th0, ll0, t["L"], t["prior"], x0, obs, obs_bin, N, n_iter, C * N, obs_std=MR.STAT_OBS_STD,
             seed=SEED + 1, trace=False)
    s = MR.summarise(r["theta_chain"][:, burn:].astype(np.float64), r["accept"][:, burn:])
    bars = MR.stat_bars(s, t)
    print(case, {k: np.round(v, 4) for k, v in s.items()}, bars)
    assert np.isfinite(r["ll_chain"]).all()
    assert bars["ok"], bars


# ----------------------------------------------------------------------------------------------------------------
# product
# ----------------------------------------------------------------------------------------------------------------
MC, MN, MITER, MBURN = 8, 64, 40, 10
MCMC_KEYS = ("probs", "mcmc/theta", "mcmc/loglik", "mcmc/accept_rate", "mcmc/prop_chol", "mcmc/mean", "mcmc/sd",
             "mcmc/quantiles", "mcmc/rhat", "theta/mean", "theta/sd", "theta/quantiles")


@pytest.fixture(scope="module")
def sampled():
    model = filter_model("ar")
    return model, model.theta_mcmc(MC, MN, MITER, MBURN)


def test_product_keys_shapes_and_by_hand_call(sampled):
    from viforssms_amd import diagnostics, ops
    model, got = sampled
    md, T, P = model.mdef, 150, 3
    assert sorted(got) == sorted(MCMC_KEYS)
    shapes = {"probs": (5,), "mcmc/theta": (MC, MITER - MBURN, P), "mcmc/loglik": (MC, MITER - MBURN),
              "mcmc/accept_rate": (MC,), "mcmc/prop_chol": (P, P), "mcmc/mean": (P,), "mcmc/sd": (P,),
              "mcmc/quantiles": (5, P), "mcmc/rhat": (P,), "theta/mean": (P,), "theta/sd": (P,),
              "theta/quantiles": (5, P)}
    for k, shp in shapes.items():
        assert got[k].shape == shp, k
    _, theta = model.sample_paths_theta(np.tile(0, model.p_local), step=model.global_step)
    draw = theta.detach().float().contiguous()
    sigma = np.cov(draw.cpu().numpy().astype(np.float64).T)
    chol = np.linalg.cholesky(2.38 ** 2 / P * sigma)
    assert np.array_equal(got["mcmc/prop_chol"], chol)
    summary = model.posterior_summary()
    for k in ("mean", "sd", "quantiles"):
        assert np.array_equal(got[f"theta/{k}"], summary[f"theta/{k}"]), k
    obs, obs_bin, x0 = (torch.as_tensor(a, device=DEV) for a in model.filter_data)
    obs, obs_bin, x0 = obs[:, :T].contiguous(), obs_bin[:, :T].contiguous(), x0.float().reshape(-1)
    seed = model.engine.seed ^ diagnostics.MCMC_SEED_XOR
    row0 = model.global_step * MC * MN * (MITER + 1)
    th = draw[:MC].contiguous()
    ll = ops.particle_filter(md.model_id, th, x0, obs, obs_bin, md.dt, md.obs_std, MN, seed, row0, cloud=False,
                             proposal="adapted").loglik
    r = ops.pmmh(md.model_id, th, ll, g(chol.astype(np.float32)), g(np.asarray(md.priors, np.float32)), x0, obs, obs_bin,
                 md.dt, md.obs_std, MN, MITER, seed, row0 + MC * MN)
    assert np.array_equal(_bits(got["mcmc/theta"]), _bits(r.theta_chain[:, MBURN:].cpu().numpy()))
    assert np.array_equal(_bits(got["mcmc/loglik"]), _bits(r.ll_chain[:, MBURN:].cpu().numpy()))
    assert np.array_equal(got["mcmc/accept_rate"], r.accept[:, MBURN:].double().mean(1).cpu().numpy())
    assert np.isfinite(got["mcmc/loglik"]).all() and 0.0 < got["mcmc/accept_rate"].mean() < 1.0
    want = [MR.split_rhat(got["mcmc/theta"][:, :, i]) for i in range(P)]
    assert np.allclose(got["mcmc/rhat"], want, rtol=1e-12, atol=0) and np.all(got["mcmc/rhat"] > 0.9)
    pooled = got["mcmc/theta"].reshape(-1, P).astype(np.float64)
    pooled[:, 2] = np.exp(got["mcmc/theta"].reshape(-1, P)[:, 2].astype(np.float64))   # theta_pos of AR
    assert np.allclose(got["mcmc/mean"], pooled.mean(0), rtol=1e-5)
    assert np.allclose(got["mcmc/quantiles"], np.quantile(pooled, got["probs"], axis=0), rtol=1e-5)


def test_product_launch_cutting_save_and_refusals(sampled, tmp_path, monkeypatch):
    from tests.parity_util import build_model
    from viforssms_amd import diagnostics, ops
    model, got = sampled
    calls = []
    real = ops.pmmh
    monkeypatch.setattr(ops, "pmmh", lambda *a, **kw: calls.append((a[11], kw.get("it0"))) or real(*a, **kw))
    monkeypatch.setattr(diagnostics, "MCMC_LAUNCH_STEPS", 150 * 7 + 3)        # seven iterations per launch
    path = str(tmp_path / "sub" / "mcmc.npz")
    cut = model.save_theta_mcmc(path, MC, MN, MITER, MBURN)
    assert calls == [(7, 0), (7, 7), (7, 14), (7, 21), (7, 28), (5, 35)]
    for k in MCMC_KEYS:
        assert np.array_equal(cut[k], got[k]), k
    with np.load(path) as z:
        assert sorted(z.files) == sorted(MCMC_KEYS)
        for k in MCMC_KEYS:
            assert np.array_equal(z[k], got[k]), k
    monkeypatch.setattr(diagnostics, "MCMC_LAUNCH_STEPS", 1)                  # at least one iteration per launch
    calls.clear()
    one = model.theta_mcmc(MC, MN, 4, 1)
    assert calls == [(1, i) for i in range(4)] and one["mcmc/theta"].shape == (MC, 3, 3)
    for kw, msg in ((dict(n_particles=96), "n_particles"), (dict(n_chains=0), "n_chains"),
                    (dict(n_chains=model.p_local + 1), "n_chains"), (dict(n_iter=5, burn_in=5), "burn_in"),
                    (dict(step_scale=0.0), "step_scale")):
        with pytest.raises(ValueError, match=msg):
            model.theta_mcmc(**{**dict(n_chains=MC, n_particles=MN, n_iter=MITER, burn_in=MBURN), **kw})
    sv = build_model("sv", 7, 40, 8, 2, 16, 5, 3, DEV, T=160, precision=0, seed=3)
    with pytest.raises(ValueError, match="SV"):
        sv.theta_mcmc(4, 64, 10, 2)


def test_main_writes_the_chains(tmp_path, monkeypatch):
    """python main.py hyperparameters.txt ... --mcmc 4 64 12 PATH: two training steps, then the .npz."""
    state = np.random.get_state()
    monkeypatch.chdir(tmp_path)
    try:
        import main
        out = str(tmp_path / "post" / "mcmc.npz")
        model = main.run([os.path.join(ROOT, "hyperparameters.txt"), "-T", "60", "-b", "30", "-k", "5", "-p", "8",
                          "-f", "4", "--steps", "2", "--no-pretrain", "--mcmc", "4", "64", "12", out])
    finally:
        np.random.set_state(state)
    assert model.global_step == 2
    with np.load(out) as z:
        assert sorted(z.files) == sorted(MCMC_KEYS)
        assert z["mcmc/theta"].shape == (4, 9, 3) and z["mcmc/quantiles"].shape == (5, 3) and z["mcmc/rhat"].shape == (3,)
