"""Writes tests/golden/svf_series.npz, the statistical case of the stochastic-volatility filter and smoother tests
(tests/svf_ref.py): numpy only.

  y            [T + 1] float32, simulated from the model at viforssms_amd.sv.PARAM_INIT with dt = 1, h_0 = -8.5,
               y_0 = 1 (T = 64); h_true [T + 1] the latent path that produced it
  grid_n       the two grid sizes of svf_ref.grid_pass on [-16, 1]
  grid_loglik  [2] log p(y_1:T | y_0, h_0) from each;  grid_ms, grid_sds [2, T] the smoothing means and sds;
               grid_mf, grid_sdf [2, T] the filtering ones
  ref_logliks  [1024] float64: the log-evidence estimates of 1024 free-running reference filters of N = 256
               (svf_ref.run_filter on default_rng(ref_seed))

usage: python -m tests.golden.make_svf_fixture [seed]"""
import sys

import numpy as np

from tests import svf_ref as R


def main(seed=0, ref_seed=11):
    y, h = R.simulate_series(R.FIX_T, R.PARAM_INIT, R.FIX_DT, R.FIX_H0, R.FIX_Y0, np.random.default_rng(seed))
    assert np.isfinite(y).all() and not np.any(y[:-1] == 0)
    y64 = y.astype(np.float64)
    sizes = (2001, 4001)
    grids = [R.grid_pass(R.PARAM_INIT, R.FIX_H0, y64, R.FIX_DT, n) for n in sizes]
    for k in ("ms", "sds"):
        print(k, "max difference between the grids:", float(np.max(np.abs(grids[0][k] - grids[1][k]))))
    print("grid loglik:", [g["loglik"] for g in grids])
    th = np.tile(np.asarray(R.PARAM_INIT), (R.FIX_K, 1))
    ref = R.run_filter(th, R.FIX_H0, y64, R.FIX_DT, R.FIX_N, np.random.default_rng(ref_seed))["loglik"]
    print(f"reference: mean {ref.mean():.4f} sd {ref.std(ddof=1):.4f}")
    np.savez(R.FIXTURE, y=y, h_true=h, seed=np.int64(seed), ref_seed=np.int64(ref_seed),
             grid_n=np.asarray(sizes, np.int64), grid_loglik=np.asarray([g["loglik"] for g in grids]),
             **{f"grid_{k}": np.stack([g[k] for g in grids]) for k in ("ms", "sds", "mf", "sdf")}, ref_logliks=ref)


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:]))
