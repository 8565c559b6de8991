"""VISSMBase.posterior_summary / save_summary / main.py --summary against the host path they replace: save_paths
writes every sample of every window as text (np.savetxt's %.18e round-trips fp32) and numpy takes the statistics of
that file.  The summary visits the same windows, draws and step, so its quantiles -- float64 interpolations between
two exact order statistics on both sides -- must equal np.quantile of the file at rtol 1e-12, and its means hold the
moments' bound |sum - ref| <= 2 B 2^-53 sum|x| (tests/test_gpu_colstat.py)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# family -> (B, M, k, n_flows, H, n_layers, fw), T, precision (0 fp32, 1 bf16), D
CASES = {"ar": ((64, 30, 5, 2, 20, 3, 4), 150, 0, 1),     # five windows
         "lv": ((32, 24, 4, 2, 16, 5, 3), 24, 1, 2)}
U = 2.0 ** -53


def _model(family):
    from tests.parity_util import build_model
    shape, T, prec, _ = CASES[family]
    return build_model(family, *shape, DEV, T=T, precision=prec, seed=3)


def _check(got, prefix, x64, probs):
    """got[prefix/...] against numpy on the samples x64 [B, n] (float64 copies of fp32 values)."""
    B = x64.shape[0]
    q = got[f"{prefix}/quantiles"].reshape(len(probs), -1)
    mean, sd = got[f"{prefix}/mean"].reshape(-1), got[f"{prefix}/sd"].reshape(-1)
    assert np.allclose(q, np.quantile(x64, probs, axis=0), rtol=1e-12, atol=0.0)
    assert np.all(np.abs(mean - x64.mean(0)) <= 2.0 * B * U * np.abs(x64).mean(0))
    # sd from E x^2 - mean^2 in float64: both terms carry the moments' bound, an absolute error in the variance
    assert np.all(np.abs(sd ** 2 - x64.var(0)) <= 8.0 * (B + 2) * U * (x64 * x64).mean(0))
    assert np.all(np.diff(q, axis=0) >= 0)


@pytest.fixture(scope="module", params=["ar", "lv"])
def summarised(request, tmp_path_factory):
    """One model per family, its save_paths file and its posterior summary (shared by the tests below)."""
    from viforssms_amd.summary import DEFAULT_PROBS
    family = request.param
    model = _model(family)
    path = str(tmp_path_factory.mktemp(family) / "paths.txt")
    model.save_paths(path)
    paths = np.loadtxt(path, ndmin=2)
    return family, model, paths, model.posterior_summary(), DEFAULT_PROBS


def test_path_bands_equal_numpy_on_the_save_paths_file(summarised):
    family, model, paths, got, probs = summarised
    (B, M, *_), T, _, D = CASES[family]
    assert paths.shape == (B, D * T)
    assert np.array_equal(got["probs"], np.asarray(probs))
    assert got["paths/mean"].shape == (D, T) and got["paths/sd"].shape == (D, T)
    assert got["paths/quantiles"].shape == (len(probs), D, T)
    assert all(got[k].dtype == np.float64 for k in ("paths/mean", "paths/sd", "paths/quantiles"))
    assert np.array_equal(got["paths/n_valid"], np.full((D, T), B))
    _check(got, "paths", paths, probs)


def test_theta_summary_equals_numpy_on_the_same_draw(summarised):
    family, model, _, got, probs = summarised
    (B, *_), _, _, _ = CASES[family]
    _, theta = model.sample_paths_theta(np.tile(0, model.p_local), step=model.global_step)
    th = theta.detach().float()
    pos = list(model.mdef.theta_pos)
    assert any(pos)
    th = torch.where(torch.tensor(pos, device=th.device), th.exp(), th).cpu().numpy()
    P = th.shape[1]
    assert got["theta/mean"].shape == (P,) and got["theta/quantiles"].shape == (len(probs), P)
    assert np.array_equal(got["theta/n_valid"], np.full(P, B))
    _check(got, "theta", th.astype(np.float64), probs)


def test_other_probs_and_their_limit(summarised):
    family, model, paths, _, _ = summarised
    probs = (0.0, 0.1, 0.5, 1.0)
    got = model.posterior_summary(probs)
    _check(got, "paths", paths, probs)
    assert np.array_equal(got["paths/quantiles"][0].reshape(-1), paths.min(0))
    assert np.array_equal(got["paths/quantiles"][-1].reshape(-1), paths.max(0))
    with pytest.raises(ValueError):
        model.posterior_summary([0.1] * 9)


def test_save_summary_round_trips(summarised, tmp_path):
    family, model, _, got, _ = summarised
    path = str(tmp_path / "sub" / "summary.npz")
    res = model.save_summary(path)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(got)
        for k in got:
            assert np.array_equal(z[k], got[k], equal_nan=True) and np.array_equal(res[k], got[k], equal_nan=True), k


def test_main_writes_the_summary(tmp_path, monkeypatch):
    """python main.py hyperparameters.txt ... --summary PATH: two training steps, then the .npz."""
    state = np.random.get_state()
    monkeypatch.chdir(tmp_path)          # main.py writes dat/, train/ and model_saves/ under the working directory
    try:
        import main
        out = str(tmp_path / "post" / "summary.npz")
        model = main.run([os.path.join(ROOT, "hyperparameters.txt"), "-T", "60", "-b", "30", "-k", "5", "-p", "8",
                          "-f", "4", "--steps", "2", "--no-pretrain", "--summary", out])
    finally:
        np.random.set_state(state)
    assert model.global_step == 2
    with np.load(out) as z:
        assert z["paths/mean"].shape == (1, 60) and z["paths/quantiles"].shape == (5, 1, 60)
        assert z["theta/mean"].shape == (3,) and z["theta/quantiles"].shape == (5, 3)
        assert np.isfinite(z["paths/quantiles"]).all() and np.all(np.diff(z["paths/quantiles"], axis=0) >= 0)
        assert np.array_equal(z["paths/n_valid"], np.full((1, 60), 8))
