"""The host side of viforssms_amd/diagnostics.py, without a GPU: the band assembler that lays the chunks' flat
[S * m] column summaries side by side as [S, T], the chunk formula, and the rank-0 .npz writer."""
import os
import types

import numpy as np
import pytest

from viforssms_amd import _lib
from viforssms_amd.diagnostics import PosteriorDiagnostics, stack_bands

Q = 5


def _part(c, S, m):
    """Chunk c's column summary, every entry its own address: 1000 c + (q S m +) d m + t."""
    flat = 1000 * c + np.arange(S * m)
    return m, {"mean": flat.astype(np.float64), "sd": flat + 0.5, "n_valid": flat.astype(np.int64),
               "quantiles": (1000 * c + np.arange(Q * S * m)).reshape(Q, S * m).astype(np.float64)}


@pytest.mark.parametrize("S", [1, 2])
def test_stack_bands_of_no_chunk(S):
    res = stack_bands("filter", [], S, Q)
    assert sorted(res) == ["filter/mean", "filter/n_valid", "filter/quantiles", "filter/sd"]
    for k in ("mean", "sd", "n_valid"):
        assert res[f"filter/{k}"].shape == (S, 0), k
    assert res["filter/quantiles"].shape == (Q, S, 0)
    assert res["filter/mean"].dtype == res["filter/sd"].dtype == res["filter/quantiles"].dtype == np.float64
    assert res["filter/n_valid"].dtype == np.int64


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("ms", [(4,), (3, 5, 1)])
def test_stack_bands_puts_every_column_at_its_step_and_coordinate(S, ms):
    res = stack_bands("forecast/obs", [_part(c, S, m) for c, m in enumerate(ms)], S, Q)
    T = sum(ms)
    assert sorted(res) == ["forecast/obs/mean", "forecast/obs/n_valid", "forecast/obs/quantiles", "forecast/obs/sd"]
    assert res["forecast/obs/mean"].shape == res["forecast/obs/sd"].shape == res["forecast/obs/n_valid"].shape == (S, T)
    assert res["forecast/obs/quantiles"].shape == (Q, S, T)
    assert res["forecast/obs/mean"].dtype == res["forecast/obs/quantiles"].dtype == np.float64
    assert res["forecast/obs/n_valid"].dtype == np.int64
    t0 = 0
    for c, m in enumerate(ms):
        for d in range(S):
            for t in range(m):
                at = 1000 * c + d * m + t
                assert res["forecast/obs/mean"][d, t0 + t] == at
                assert res["forecast/obs/sd"][d, t0 + t] == at + 0.5
                assert res["forecast/obs/n_valid"][d, t0 + t] == at
                for q in range(Q):
                    assert res["forecast/obs/quantiles"][q, d, t0 + t] == at + q * S * m
        t0 += m


@pytest.mark.parametrize("model_id", sorted(_lib.MODEL_S))
def test_chunk_steps(model_id):
    stub = types.SimpleNamespace(mdef=types.SimpleNamespace(model_id=model_id))
    steps = PosteriorDiagnostics._chunk_steps
    assert steps(stub, 64 * 1024) % 64 == 0 and steps(stub, 64 * 1024) > 64
    assert steps(stub, 10 ** 6 * 1024) == 64
    assert steps(stub, 0) == steps(stub, 1)
    S = _lib.MODEL_S[model_id]
    for rows in (1, 100, 64 * 1024):
        n = steps(stub, rows)
        assert 4 * S * rows * n <= (256 << 20) < 4 * S * rows * (n + 64)


def test_save_npz_is_rank_zeros(tmp_path):
    res = {"probs": np.linspace(0.0, 1.0, Q), "filter/n_valid": np.arange(6).reshape(2, 3)}
    path = str(tmp_path / "not" / "yet" / "there.npz")
    rank = lambda r: types.SimpleNamespace(dist=types.SimpleNamespace(rank=r))
    assert PosteriorDiagnostics._save_npz(rank(1), path, res) is res
    assert not os.path.exists(os.path.dirname(path))
    assert PosteriorDiagnostics._save_npz(rank(0), path, res) is res
    with np.load(path) as z:
        assert sorted(z.files) == sorted(res)
        for k in res:
            assert np.array_equal(z[k], res[k]) and z[k].dtype == res[k].dtype
