"""Time the particle smoother's backward simulation (vissm_particle_smooth) against a torch restatement of the same
loop.

Two shapes, the horizon cut into launches as VISSMBase.particle_smoother cuts it (walked last to first, chained through
x_first); the clouds are the ones ops.particle_filter writes for scripts/bench_filter.py's data, outside the timing:

  AR   T = 5000, K = 64 filters, N = 1024 particles, M = 1024 trajectories per filter   (1024 steps per launch)
  LV   T = 1000, K = 64 filters, N = 1024 particles, M = 256 trajectories per filter    (512 steps per launch)

Timed on each, with device events around --reps back-to-back passes over the whole horizon, warmed up, in alternating
runs, reported per pass:

  kernel   ops.particle_smooth over the kept clouds (paths [K M, S, T] written: the production path of the bands)
  torch    the parent has no such kernel, so the yardstick is the same backward loop on [K, M, N] tensors: the
           per-particle part once per step, the pair log-weights, q = floor(exp(logw - m) 2^40) in int64, cumsum,
           tau from 25-bit halves of W (int64 cannot hold the 82-bit product), searchsorted, gather.  The selection
           words are pre-drawn by torch.randint outside the timed window; nothing is stored per step.  It walks the
           last --torch-steps steps only (0: all) and is reported per step and scaled to the horizon, marked so.

Reported per shape: median, minimum and maximum milliseconds over the runs, pairs = K M N T, the exps per pair as built
(1 + 64 / N), the floor the transcendental issue rate puts under them (derived: 8 cycles per wave-instruction for one
wave on a SIMD, 1024 SIMDs at 2.4 GHz -- MI355X_MICROARCH.md's constants -- not measured) and the kernel's share of
it, and the means over the trajectories of both at three steps (they share the clouds but not the selection words,
so they agree in distribution only).

    python scripts/bench_smooth.py [--runs 5] [--reps 1] [--torch-steps 200] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_filter as BF      # the data, the parameters and the timer of the filter's benchmark

DEV = "cuda:0"
SEED = 8765
SMOOTH_M = {"ar": 1024, "lv": 256}
EXP_ISSUE_CYCLES, N_SIMD, CLOCK_HZ = 8.0, 1024, 2.4e9      # derived floor: one wave on a SIMD, v_exp_f32


def filter_clouds(name):
    """[(t0, cloud [K N, S, m])] of the filter over the benchmark's data, and theta [K, P]."""
    from viforssms_amd import ops
    model, T, K, N, chunk, dt, sd, x_true, th_true = BF.CASES[name]
    obs_h, bin_h = BF.make_data(name, T)
    obs, obs_bin = torch.as_tensor(obs_h, device=DEV), torch.as_tensor(bin_h, device=DEV)
    rng = np.random.default_rng(0)
    th = torch.as_tensor((np.asarray(th_true) + rng.uniform(-0.02, 0.02, (K, len(th_true)))).astype(np.float32),
                         device=DEV)
    state = torch.as_tensor(np.tile(np.asarray(x_true, np.float32), (K * N, 1)), device=DEV)
    ll, clouds = None, []
    for t0 in range(0, T, chunk):
        r = ops.particle_filter(model, th, state, obs, obs_bin, dt, sd, N, BF.SEED, 0, t0=t0, loglik_in=ll, cloud=True,
                                H=min(chunk, T - t0))
        state, ll = r.state_end, r.loglik
        clouds.append((t0, r.cloud))
    assert torch.isfinite(ll).all(), "a filter died: the benchmark's clouds would hold NaN"
    return th, clouds


def run_kernel(model, th, clouds, dt, M, keep=None):
    from viforssms_amd import ops
    x_next = None
    for t0, cloud in reversed(clouds):
        r = ops.particle_smooth(model, th, cloud, dt, M, SEED, 0, t0=t0, x_next=x_next)
        x_next = r.x_first
        if keep is not None:
            keep.append(r.paths)
    return x_next


def run_torch(model, th, clouds, dt, M, K, N, U, steps, keep=None):
    """The restatement over the last `steps` steps: U [T, K, M] int64 selection words."""
    S = clouds[0][1].shape[1]
    rows = (torch.arange(K, device=DEV) * N).view(K, 1)
    e = th.exp()
    xt, done = None, 0
    for t0, cloud in reversed(clouds):
        for i in range(cloud.shape[2] - 1, -1, -1):
            if done == steps:
                return xt
            x = cloud[:, :, i].view(K, N, S)
            if xt is None:
                lw = torch.zeros(K, M, N, device=DEV)
            elif model == 0:
                mean = th[:, 1:2] * x[:, :, 0] + th[:, 0:1]
                z = (xt[:, :, 0].unsqueeze(2) - mean.unsqueeze(1)) * (-th[:, 2]).exp().view(K, 1, 1)
                lw = -0.5 * z * z
            else:
                x1, x2 = x[:, :, 0], x[:, :, 1]
                Bv = e[:, 1:2] * (x1 * x2)
                A, Cc = e[:, 0:1] * x1 + Bv, Bv + e[:, 2:3] * x2
                inv = 1.0 / (dt * (A * Cc - Bv * Bv))
                q1 = xt[:, :, 0].unsqueeze(2) - (x1 + dt * (e[:, 0:1] * x1 - Bv)).unsqueeze(1)
                q2 = xt[:, :, 1].unsqueeze(2) - (x2 + dt * (Bv - e[:, 2:3] * x2)).unsqueeze(1)
                quad = (inv * Cc).unsqueeze(1) * q1 * q1 + 2.0 * (inv * Bv).unsqueeze(1) * q1 * q2 + \
                    (inv * A).unsqueeze(1) * q2 * q2
                lw = (-0.5 * (dt * dt * (A * Cc - Bv * Bv)).log()).unsqueeze(1) - 0.5 * quad
            m = lw.max(2, keepdim=True).values
            q = ((lw - m).exp() * 2.0 ** 40).to(torch.int64)
            C = q.cumsum(2)
            W = C[:, :, -1]
            u = U[t0 + i]
            tau = (u * (W >> 25) + ((u * (W & ((1 << 25) - 1))) >> 25)) >> 7
            idx = torch.searchsorted(C, tau.unsqueeze(2), right=True).squeeze(2).clamp_(max=N - 1)
            xt = cloud[:, :, i][(rows + idx).view(-1)].view(K, M, S)
            if keep is not None:
                keep.append(xt)
            done += 1
    return xt


def bench_case(name, runs, reps, torch_runs, torch_steps):
    from viforssms_amd import _lib
    model, T, K, N, chunk, dt, sd, x_true, th_true = BF.CASES[name]
    M, S = SMOOTH_M[name], len(x_true)
    th, clouds = filter_clouds(name)
    steps = T if torch_steps <= 0 else min(T, torch_steps)
    U = torch.randint(0, 1 << 32, (T, K, M), device=DEV, dtype=torch.int64)
    kfn = lambda: run_kernel(model, th, clouds, dt, M)
    tfn = lambda: run_torch(model, th, clouds, dt, M, K, N, U, steps)
    kfn()                                                    # warm-up of every shape the timed runs use
    run_torch(model, th, clouds, dt, M, K, N, U, 4)
    ms_k, ms_t = [], []
    for i in range(max(runs, torch_runs)):                   # alternating
        if i < runs:
            ms_k.append(BF.timed(kfn, reps))
        if i < torch_runs:
            ms_t.append(BF.timed(tfn))
    kp, tp = [], []
    run_kernel(model, th, clouds, dt, M, kp)
    run_torch(model, th, clouds, dt, M, K, N, U, min(steps, 64), tp)
    kpaths = torch.cat(list(reversed(kp)), 2)                # [K M, S, T]
    assert torch.isfinite(kpaths).all()
    at = [T - 1, T - 1 - min(steps, 64) // 2, T - min(steps, 64)]
    pairs = K * M * N * T
    exps = 1.0 + 64.0 / N
    floor_ms = pairs * exps / 64.0 * EXP_ISSUE_CYCLES / N_SIMD / CLOCK_HZ * 1e3
    res = {"case": name, "model": model, "T": T, "K": K, "N": N, "M": M, "steps_per_launch": chunk,
           "launches": len(clouds), "passes_per_timed_window": reps, "pairs": pairs, "exps_per_pair": exps,
           "cloud_bytes": K * N * S * T * 4, "paths_bytes": K * M * S * T * 4,
           "lds_bytes_per_block": int(_lib.load().vissm_particle_smooth_lds_bytes(model, N, M)),
           "blocks_per_launch": K * M // 64, "kernel": BF.stats(ms_k),
           "torch_steps_timed": steps, "torch": BF.stats(ms_t),
           "kernel_mean_at": {str(t): float(kpaths[:, 0, t].mean()) for t in at},
           "torch_mean_at": {str(t): float(tp[T - 1 - t][:, :, 0].mean()) for t in at}}
    k_ms = res["kernel"]["median_ms"]
    res["kernel_ns_per_pair"] = k_ms * 1e6 / pairs
    res["derived_exp_floor_ms"] = floor_ms
    res["kernel_share_of_derived_floor"] = floor_ms / k_ms
    res["torch_ms_per_step"] = res["torch"]["median_ms"] / steps
    res["torch_scaled_to_horizon_ms"] = res["torch_ms_per_step"] * T
    res["torch_scaled_is_extrapolated"] = steps < T
    res["torch_over_kernel"] = res["torch_scaled_to_horizon_ms"] / k_ms
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=1, help="passes over the horizon per timed window (kernel)")
    ap.add_argument("--torch-runs", type=int, default=2)
    ap.add_argument("--torch-steps", type=int, default=200, help="steps the restatement walks (0: the whole horizon)")
    ap.add_argument("--cases", default="ar,lv")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_smooth.py needs the GPU: there is nothing to time without it")
    res = {"cases": [bench_case(c, args.runs, args.reps, args.torch_runs, args.torch_steps)
                     for c in args.cases.split(",")]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
