"""VISSMBase.forecast / save_forecast / main.py --forecast: the posterior-predictive bands equal numpy's statistics of
ops.sde_simulate called by hand on the same draw (the last window of save_paths / posterior_summary, its theta and
its path's last state) with the documented Philox key and row.  The quantiles are float64 interpolations between two
exact order statistics on both sides (rtol 1e-12); the moments hold tests/test_gpu_summary.py's bounds; n_valid is
the count of non-NaN entries (a trajectory that left the model's domain is NaN from there on)."""
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# family -> (B, M, k, n_flows, H, n_layers, fw), T, precision, D: the shapes of tests/test_gpu_summary.py
CASES = {"ar": ((64, 30, 5, 2, 20, 3, 4), 150, 0, 1),
         "lv": ((32, 24, 4, 2, 16, 5, 3), 24, 1, 2)}
U = 2.0 ** -53
HORIZON = 37
GROUP_KEYS = ("mean", "sd", "quantiles", "n_valid")


def _model(family):
    from tests.parity_util import build_model, pin_theta
    shape, T, prec, _ = CASES[family]
    model = build_model(family, *shape, DEV, T=T, precision=prec, seed=3)
    if family == "lv":
        # build_model's random q(theta) draws log-rates ~ N(0, 1): e^th1 ~ 1 against the generator's 0.0025, and
        # every trajectory leaves the positive orthant at its first step.  Put q(theta) where a fitted model has it:
        # the generator's log-rates within a few percent.
        from tests.sim_util import LV, TRUE_THETA
        pin_theta(model, TRUE_THETA[LV])
    return model


def _by_hand(model, H, obs=False):
    """x (and y) [B, D * H] float64 from ops.sde_simulate on the last window's draw."""
    from viforssms_amd import ops
    from viforssms_amd.vi_ssm import FORECAST_SEED_XOR
    md = model.mdef
    last = np.arange(0, model.target_len(), model.batch_dims)[-1]
    x, theta = model.sample_paths_theta(np.tile(last, model.p_local), step=model.global_step)
    xs, ys, _ = ops.sde_simulate(md.model_id, theta.float().contiguous(), x[:, :, -1].float().contiguous(), H, md.dt,
                                 model.engine.seed ^ FORECAST_SEED_XOR, model.global_step * model.p,
                                 obs_std=md.obs_std if obs else None)
    flat = lambda v: v.reshape(v.shape[0], -1).cpu().numpy().astype(np.float64)
    return flat(xs), (flat(ys) if obs else None)


def _check(got, prefix, x64, probs, D, H):
    B = x64.shape[0]
    n = np.isfinite(x64).sum(0)
    assert not np.isinf(x64).any()
    assert got[f"{prefix}/mean"].shape == (D, H) and got[f"{prefix}/sd"].shape == (D, H)
    assert got[f"{prefix}/quantiles"].shape == (len(probs), D, H) and got[f"{prefix}/n_valid"].shape == (D, H)
    assert np.array_equal(got[f"{prefix}/n_valid"].reshape(-1), n)
    q = got[f"{prefix}/quantiles"].reshape(len(probs), -1)
    mean, sd = got[f"{prefix}/mean"].reshape(-1), got[f"{prefix}/sd"].reshape(-1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)     # all-NaN columns
        rq, rmean, rvar = np.nanquantile(x64, probs, axis=0), np.nanmean(x64, 0), np.nanvar(x64, 0)
        rabs, rsq = np.nanmean(np.abs(x64), 0), np.nanmean(x64 * x64, 0)
    some = n > 0
    assert np.isnan(q[:, ~some]).all() and np.isnan(mean[~some]).all() and np.isnan(sd[~some]).all()
    assert np.allclose(q[:, some], rq[:, some], rtol=1e-12, atol=0.0)
    assert np.all(np.abs(mean - rmean)[some] <= (2.0 * B * U * rabs)[some])
    assert np.all(np.abs(sd ** 2 - rvar)[some] <= (8.0 * (B + 2) * U * rsq)[some])
    assert np.all(np.diff(q[:, some], axis=0) >= 0)


@pytest.fixture(scope="module", params=["ar", "lv"])
def forecasted(request):
    """One model per family, its default forecast and the by-hand simulation (shared by the tests below)."""
    from viforssms_amd.summary import DEFAULT_PROBS
    family = request.param
    model = _model(family)
    return family, model, model.forecast(HORIZON), _by_hand(model, HORIZON)[0], DEFAULT_PROBS


def test_bands_equal_numpy_on_the_by_hand_simulation(forecasted):
    family, model, got, x64, probs = forecasted
    (B, *_), T, _, D = CASES[family]
    assert x64.shape == (B, D * HORIZON)
    assert sorted(got) == sorted(["probs", "forecast/start"] + [f"forecast/{k}" for k in GROUP_KEYS])
    assert np.array_equal(got["probs"], np.asarray(probs)) and int(got["forecast/start"]) == T == model.target_len()
    assert all(got[f"forecast/{k}"].dtype == np.float64 for k in ("mean", "sd", "quantiles"))
    assert (got["forecast/n_valid"] > 0).any(), "every trajectory died at once: nothing is compared"
    print(f"{family}: n_valid from {got['forecast/n_valid'].max()} down to {got['forecast/n_valid'].min()} of {B}")
    _check(got, "forecast", x64, probs, D, HORIZON)


def test_chunking_changes_nothing(forecasted):
    family, model, got, _, _ = forecasted
    for chunk in (5, 36, 64):
        res = model.forecast(HORIZON, chunk=chunk)
        assert sorted(res) == sorted(got)
        for k in got:
            if k.endswith("/mean") or k.endswith("/sd"):
                continue
            assert np.array_equal(res[k], got[k], equal_nan=True), (chunk, k)
        # the samples are bitwise the same, so each column's moments are too: same kernel, same rows
        assert np.array_equal(res["forecast/mean"], got["forecast/mean"], equal_nan=True), chunk
        assert np.array_equal(res["forecast/sd"], got["forecast/sd"], equal_nan=True), chunk
    assert model.forecast_chunk() % 64 == 0 and model.forecast_chunk() >= 64
    with pytest.raises(ValueError):
        model.forecast(HORIZON, chunk=0)


def test_observation_bands(forecasted):
    family, model, got, _, probs = forecasted
    (B, *_), _, _, D = CASES[family]
    res = model.forecast(HORIZON, obs=True, chunk=16)
    assert sorted(res) == sorted(list(got) + [f"forecast/obs/{k}" for k in GROUP_KEYS])
    for k in GROUP_KEYS:
        assert res[f"forecast/obs/{k}"].shape == got[f"forecast/{k}"].shape
    n = res["forecast/obs/n_valid"]
    assert np.array_equal(n, res["forecast/n_valid"])       # an observation is NaN exactly where its state is
    q = res["forecast/obs/quantiles"]
    assert np.isfinite(q[:, n > 0]).all() and np.isfinite(res["forecast/obs/mean"][n > 0]).all()
    assert np.isfinite(res["forecast/obs/sd"][n > 0]).all()
    assert np.all(np.diff(q[:, n > 0], axis=0) >= 0)
    x64, y64 = _by_hand(model, HORIZON, obs=True)
    _check(res, "forecast/obs", y64, probs, D, HORIZON)
    _check(res, "forecast", x64, probs, D, HORIZON)


def test_empty_horizon_other_probs_and_refusals(forecasted):
    family, model, got, x64, _ = forecasted
    (B, *_), T, _, D = CASES[family]
    res = model.forecast(0, obs=True)
    assert res["forecast/mean"].shape == (D, 0) and res["forecast/quantiles"].shape == (5, D, 0)
    assert res["forecast/obs/n_valid"].shape == (D, 0) and res["forecast/n_valid"].dtype == np.int64
    assert int(res["forecast/start"]) == T
    probs = (0.0, 0.5, 1.0)
    _check(model.forecast(HORIZON, probs), "forecast", x64, probs, D, HORIZON)
    with pytest.raises(ValueError):
        model.forecast(-1)
    with pytest.raises(ValueError):
        model.forecast(5, [0.1] * 9)


def test_sv_has_no_observation_forecast():
    from tests.parity_util import build_model
    # tests/test_gpu_windows.py's SV shape
    model = build_model("sv", 7, 40, 8, 2, 16, 5, 3, DEV, T=160, precision=0, seed=3)
    with pytest.raises(ValueError, match="SV"):
        model.forecast(5, obs=True)
    res = model.forecast(5)
    assert res["forecast/quantiles"].shape == (5, 2, 5) and int(res["forecast/start"]) == 160


def test_save_forecast_round_trips(forecasted, tmp_path):
    family, model, got, _, _ = forecasted
    path = str(tmp_path / "sub" / "forecast.npz")
    res = model.save_forecast(path, HORIZON)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(got)
        for k in got:
            assert np.array_equal(z[k], got[k], equal_nan=True) and np.array_equal(res[k], got[k], equal_nan=True), k


def test_main_writes_the_forecast(tmp_path, monkeypatch):
    """python main.py hyperparameters.txt ... --forecast 20 PATH: two training steps, then the .npz."""
    state = np.random.get_state()
    monkeypatch.chdir(tmp_path)          # main.py writes dat/, train/ and model_saves/ under the working directory
    try:
        import main
        out = str(tmp_path / "post" / "forecast.npz")
        model = main.run([os.path.join(ROOT, "hyperparameters.txt"), "-T", "60", "-b", "30", "-k", "5", "-p", "8",
                          "-f", "4", "--steps", "2", "--no-pretrain", "--forecast", "20", out])
    finally:
        np.random.set_state(state)
    assert model.global_step == 2
    with np.load(out) as z:
        assert z["forecast/quantiles"].shape == (5, 1, 20) and z["forecast/mean"].shape == (1, 20)
        assert int(z["forecast/start"]) == 60
        assert np.array_equal(z["forecast/n_valid"], np.full((1, 20), 8))
        assert np.isfinite(z["forecast/quantiles"]).all() and np.all(np.diff(z["forecast/quantiles"], axis=0) >= 0)
