"""bench.py's command line and output dump, on CPU: --full is off by default and gates the legs that take runs of
their own; dump_outputs writes float32 / float64 .npy files and samples large arrays at fixed seeded indices."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_plain_run_is_lean_by_default():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert a.full is False and a.dump_outputs is None
    assert (a.steps, a.warmup, a.gpus) == (7, 3, 1)
    # the legs keep their own switches; they take effect only under --full
    assert (a.parity_line, a.cpu_baseline, a.families) == ("auto", "auto", "auto")
    f = bench.parse_args(["--full", "--families", "off", "--dump-outputs", "d"])
    assert f.full is True and f.families == "off" and f.dump_outputs == "d"


def test_dump_outputs_dtypes_and_fixed_sample(tmp_path):
    n = bench.DUMP_MAX_ELEMS
    big = torch.arange(3 * n, dtype=torch.float32).reshape(3, n).t()  # non-contiguous, above the cap
    arrays = {"big": big, "small": torch.ones(5, 2, dtype=torch.bfloat16), "f64": torch.full((4,), 0.1, dtype=torch.float64),
              "scalar": 2.5, "absent": None}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(got) == ["big", "f64", "scalar", "small"]
    assert got["small"].dtype == np.float32 and got["small"].shape == (5, 2)
    assert got["f64"].dtype == np.float64 and got["f64"][0] == 0.1
    assert got["scalar"].dtype == np.float32 and float(got["scalar"]) == 2.5
    idx = np.sort(np.random.default_rng(0).integers(0, 3 * n, n))
    assert got["big"].dtype == np.float32 and got["big"].shape == (n,)
    assert np.array_equal(got["big"], big.contiguous().view(-1).numpy()[idx])
    assert np.array_equal(got["big"], np.load(tmp_path / "b" / "big.npy"))
    assert sum(a.nbytes for a in got.values()) <= 64 * 2 ** 20
