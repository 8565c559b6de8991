"""Time the stochastic-volatility particle filter and smoother (vissm_sv_filter, vissm_sv_smooth) beside their closest
relatives on the same machine in the same session, and measure the spread of the log-evidence estimate.

The parent commit has no SV filter, so the yardstick is the AR fully adapted filter at the same K = 64 filters of
N = 1024 particles over the same T = 1508 steps with every step observed: the same state size, barriers, Philox stream
and LDS tile; SV adds an exp and a log per step and particle.  The SV series is dat/SV.dat (1509 values) with theta
within 0.02 of viforssms_amd.sv.PARAM_INIT and h_0 = -8.5; the AR series is simulated at its generator's parameters.

  sv / ar             the filter over the whole horizon, cloud written; *_nocloud: cloud = NULL
  sv_smooth / ar_smooth   M = 64 trajectories per filter backward over the kept cloud (the filter is not in the time)
  sv_common_theta     mean and sd of loglik over the K filters at theta = PARAM_INIT for all of them: the estimator's
                      own spread (not after a training run: theta is the pretraining target)
  after_training      with --train-steps S: the SV config pretrained and trained S steps, then the spread of
                      filter/loglik over volatility_filter(64, 1024) on the fitted q(theta)'s own draws

Device events around --reps back-to-back passes, warmed up, --runs alternating runs, median and range.

    python scripts/bench_sv_filter.py [--runs 5] [--reps 3] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_filter import DEV, SEED, stats, timed  # noqa: E402

K, N, M, CHUNK = 64, 1024, 64, 512
AR_THETA, AR_X0 = [5.0, 0.5, float(np.log(3.0))], 10.0


def sv_filter(th, h0, y, cloud, keep=None):
    from viforssms_amd import ops
    T = y.shape[0] - 1
    state, ll = h0, None
    for t0 in range(0, T, CHUNK):
        r = ops.sv_filter(th, state, y, 1.0, N, SEED, 0, t0=t0, loglik_in=ll, cloud=cloud, H=min(CHUNK, T - t0))
        state, ll = r.state_end, r.loglik
        if keep is not None:
            keep.append((t0, r.cloud))
    return ll


def ar_filter(th, x0, obs, obs_bin, cloud, keep=None):
    from viforssms_amd import ops
    T = obs.shape[1]
    state, ll = x0, None
    for t0 in range(0, T, CHUNK):
        r = ops.particle_filter(0, th, state, obs, obs_bin, 1.0, 1.0, N, SEED, 0, t0=t0, loglik_in=ll, cloud=cloud,
                                H=min(CHUNK, T - t0), proposal="adapted")
        state, ll = r.state_end, r.loglik
        if keep is not None:
            keep.append((t0, r.cloud))
    return ll


def smooth(clouds, one):
    """Backward through the chunks, last to first; one(t0, cloud, x_next) -> x_first."""
    x_next = None
    for t0, cloud in reversed(clouds):
        x_next = one(t0, cloud, x_next)
    return x_next


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="passes over the horizon per timed window")
    ap.add_argument("--out", default=None)
    ap.add_argument("--train-steps", type=int, default=0,
                    help="then pretrain and train the SV config this many steps and report the spread of filter/loglik "
                         "over volatility_filter(64, 1024) (0: skip)")
    args = ap.parse_args()
    if args.out:
        args.out = os.path.abspath(args.out)
    if not torch.cuda.is_available():
        sys.exit("bench_sv_filter.py needs the GPU: there is nothing to time without it")
    from viforssms_amd import _lib, ops
    from viforssms_amd.data import load_sv
    from viforssms_amd.sv import PARAM_INIT
    y_h = np.asarray(load_sv(), np.float32)
    T = y_h.shape[0] - 1
    rng = np.random.default_rng(0)
    y = torch.as_tensor(y_h, device=DEV)
    th_sv = torch.as_tensor((np.asarray(PARAM_INIT) + rng.uniform(-0.02, 0.02, (K, 4))).astype(np.float32), device=DEV)
    th_one = torch.as_tensor(np.tile(np.asarray(PARAM_INIT, np.float32), (K, 1)), device=DEV)
    h0 = torch.full((1,), -8.5, device=DEV)
    x, xs = AR_X0, np.zeros(T)
    for t in range(T):
        x = AR_THETA[1] * x + AR_THETA[0] + 3.0 * rng.standard_normal()
        xs[t] = x
    obs = torch.as_tensor((xs + rng.standard_normal(T)).astype(np.float32)[None, :], device=DEV)
    obs_bin = torch.ones_like(obs)
    th_ar = torch.as_tensor((np.asarray(AR_THETA) + rng.uniform(-0.02, 0.02, (K, 3))).astype(np.float32), device=DEV)
    x0 = torch.full((1,), AR_X0, device=DEV)

    sv_clouds, ar_clouds = [], []
    sv_filter(th_sv, h0, y, True, sv_clouds)
    ar_filter(th_ar, x0, obs, obs_bin, True, ar_clouds)
    sv_one = lambda t0, c, xn: ops.sv_smooth(th_sv, c, y, 1.0, M, SEED ^ 1, 0, t0=t0, x_next=xn).x_first
    ar_one = lambda t0, c, xn: ops.particle_smooth(0, th_ar, c, 1.0, M, SEED ^ 1, 0, t0=t0, x_next=xn).x_first
    fns = {"sv": lambda: sv_filter(th_sv, h0, y, True), "ar": lambda: ar_filter(th_ar, x0, obs, obs_bin, True),
           "sv_nocloud": lambda: sv_filter(th_sv, h0, y, False),
           "ar_nocloud": lambda: ar_filter(th_ar, x0, obs, obs_bin, False),
           "sv_smooth": lambda: smooth(sv_clouds, sv_one), "ar_smooth": lambda: smooth(ar_clouds, ar_one)}
    for f in fns.values():
        f()
    ms = {k: [] for k in fns}
    for _ in range(args.runs):        # alternating
        for k, f in fns.items():
            ms[k].append(timed(f, args.reps if "smooth" not in k else 1))
    lib = _lib.load()
    res = {"T": T, "K": K, "N": N, "M": M, "steps_per_launch": CHUNK, "passes_per_timed_window": args.reps,
           "sv_filter_lds_bytes": int(lib.vissm_sv_filter_lds_bytes(N)),
           "ar_filter_lds_bytes": int(lib.vissm_particle_filter_adapted_lds_bytes(0, N)),
           "sv_smooth_lds_bytes": int(lib.vissm_sv_smooth_lds_bytes(N, M)),
           "ar_smooth_lds_bytes": int(lib.vissm_particle_smooth_lds_bytes(0, N, M)),
           **{k: stats(v) for k, v in ms.items()}}
    for a in ("", "_nocloud", "_smooth"):
        res[f"sv_over_ar{a}"] = res["sv" + a]["median_ms"] / res["ar" + a]["median_ms"]
    for name, ll in (("sv_common_theta", sv_filter(th_one, h0, y, False)), ("sv_jittered_theta", fns["sv_nocloud"]()),
                     ("ar_jittered_theta", fns["ar_nocloud"]())):
        ll = ll.cpu().numpy()
        fin = ll[np.isfinite(ll)]
        res[name] = {"finite": int(fin.size), "mean": float(fin.mean()) if fin.size else None,
                     "sd": float(fin.std(ddof=1)) if fin.size > 1 else None}
    def emit():
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")

    emit()
    if args.train_steps > 0:
        # the product path at the SV config shape: pretraining, a short training run, then volatility_filter(64, 1024)
        # on the fitted q(theta)'s own draws (the spread is then theta's and the estimator's together)
        import tempfile
        from viforssms_amd import sv
        with tempfile.TemporaryDirectory() as tmp:      # the driver writes its event files and checkpoints to the cwd
            cwd = os.getcwd()
            os.chdir(tmp)
            try:
                model = sv.run(["--steps", str(args.train_steps)])
                got = model.volatility_filter(K, N)
            finally:
                os.chdir(cwd)
        ll = got["filter/loglik"]
        fin = ll[np.isfinite(ll)]
        res["after_training"] = {"train_steps": args.train_steps, "finite": int(fin.size),
                                 "mean": float(fin.mean()) if fin.size else None,
                                 "sd": float(fin.std(ddof=1)) if fin.size > 1 else None,
                                 "min_ess": float(np.nanmin(got["filter/ess"])),
                                 "theta_sd": [float(v) for v in got["filter/theta"].std(0, ddof=1)]}
        emit()


if __name__ == "__main__":
    main()
