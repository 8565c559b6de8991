"""Time the particle filter (vissm_particle_filter) against a torch restatement of the same loop.

Two shapes, the horizon cut into launches as VISSMBase.particle_filter cuts it (chained through state_end and loglik):

  AR   T = 5000, K = 64 filters, N = 1024 particles, about 70 % of the steps observed   (1024 steps per launch)
  LV   T = 1000, K = 64 filters, N = 1024 particles, both species observed every 10th step   (512 steps per launch)

Timed on each, with device events around --reps back-to-back passes over the whole horizon, warmed up, in alternating
runs, reported per pass:

  kernel   ops.particle_filter with the cloud [K N, S, T] written (the production path of the filtering bands)
  nocloud  the same with cloud = NULL: the chain, the weights and the resampling alone, to separate them from the stores
  torch    the parent has no such kernel, so the yardstick is the same loop on [K, N] tensors: the step of
           csrc/sim_math.hpp with the dead-row rule, the log-weights, q = floor(exp(logw - m) 2^40) in int64, cumsum,
           the thresholds from 25-bit halves of W (int64 cannot hold the 84-bit product), searchsorted, gather.  The
           normals are pre-drawn by ops.normal_base and the resampling integers by torch.randint outside the timed
           window; nothing is stored per step but the running log-likelihood.

Reported per shape: median, minimum and maximum milliseconds of each over --runs runs, the bytes the kernel writes
(K N S T 4, the cloud) over the difference kernel - nocloud, and the mean and sd over the K filters of the kernel's
and the restatement's log-likelihood estimates (they share the normals but not the resampling integers, so they
agree in distribution only).

    python scripts/bench_filter.py [--runs 5] [--reps 3] [--out FILE.json]
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

DEV = "cuda:0"
SEED = 4321
HALF_LOG_2PI = 0.9189385332046727
# model id, T, K, N, steps per launch, dt, obs_std, start state, raw theta (the generators' true values)
CASES = {"ar": (0, 5000, 64, 1024, 1024, 1.0, 1.0, [10.0], [5.0, 0.5, float(np.log(3.0))]),
         "lv": (1, 1000, 64, 1024, 512, 0.1, 1.0, [100.0, 100.0], [float(v) for v in np.log([0.5, 0.0025, 0.3])])}


def make_data(name, T):
    """obs, obs_bin [S, T] float32 from one simulated path at the true parameters."""
    if name == "lv":
        from viforssms_amd.data import lv_data_gen
        obs, obs_bin, _, _ = lv_data_gen(T, dt=0.1, obs_every=10, seed=0)
        return obs, obs_bin
    rng = np.random.default_rng(0)
    x, xs = 10.0, np.zeros(T)
    for t in range(T):
        x = 0.5 * x + 5.0 + 3.0 * rng.standard_normal()
        xs[t] = x
    b = (rng.uniform(size=T) < 0.7).astype(np.float32)
    y = np.where(b > 0, xs + rng.standard_normal(T), 0.0).astype(np.float32)
    return y[None, :], b[None, :]


def run_kernel(model, th, x0, obs, obs_bin, N, chunk, dt, sd, cloud):
    from viforssms_amd import ops
    T = obs.shape[1]
    state, ll = x0, None
    for t0 in range(0, T, chunk):
        r = ops.particle_filter(model, th, state, obs, obs_bin, dt, sd, N, SEED, 0, t0=t0, loglik_in=ll, cloud=cloud,
                                H=min(chunk, T - t0))
        state, ll = r.state_end, r.loglik
    return ll


def torch_step(model, x, th, dt, n):
    """One Euler-Maruyama step on [B, S] tensors (the formulas of csrc/sim_math.hpp), dead rows NaN."""
    if model == 0:
        nx = (th[:, 1] * x[:, 0] + th[:, 0] + th[:, 2].exp() * n[:, 0]).unsqueeze(1)
        ok = torch.isfinite(nx).all(1, keepdim=True)
    else:
        e = th.exp()
        x1, x2 = x[:, 0], x[:, 1]
        Bv = e[:, 1] * (x1 * x2)
        A, Cc = e[:, 0] * x1 + Bv, Bv + e[:, 2] * x2
        a = A.sqrt()
        b = -Bv / a
        c = (Cc - b * b).sqrt()
        sq = dt ** 0.5
        nx = torch.stack([x1 + dt * (e[:, 0] * x1 - Bv) + sq * a * n[:, 0],
                          x2 + dt * (Bv - e[:, 2] * x2) + sq * (b * n[:, 0] + c * n[:, 1])], 1)
        ok = (torch.isfinite(nx) & (nx > 0)).all(1, keepdim=True)
    return torch.where(ok, nx, torch.full_like(nx, float("nan")))


def run_torch(model, th_rows, x0, obs_h, bin_h, obs, normals, U, K, N, dt, sd):
    """The restatement: normals a list of time-major [m, K N, S] tensors, U [T, K] int64 resampling integers."""
    S = x0.shape[1]
    x = x0.clone()
    ll = torch.zeros(K, dtype=torch.float64, device=x.device)
    log2n = N.bit_length() - 1
    j24 = torch.arange(N, device=x.device, dtype=torch.int64) << 24
    rows = (torch.arange(K, device=x.device) * N).unsqueeze(1)
    const = 40.0 * np.log(2.0) + np.log(N)
    lsd = float(np.log(sd))
    t = 0
    for nn in normals:
        for i in range(nn.shape[0]):
            x = torch_step(model, x, th_rows, dt, nn[i])
            if bin_h[:, t].any():
                lw = torch.zeros(K * N, device=x.device)
                for d in range(S):
                    if bin_h[d, t] != 0:
                        z = (x[:, d] - obs[d, t]) / sd
                        lw = lw + float(bin_h[d, t]) * (-0.5 * z * z - lsd - HALF_LOG_2PI)
                lw = torch.where(torch.isnan(lw), torch.full_like(lw, float("-inf")), lw).view(K, N)
                m = lw.max(1, keepdim=True).values
                q = ((lw - m).exp() * 2.0 ** 40).to(torch.int64)
                C = q.cumsum(1)
                W = C[:, -1:]
                a = j24 + U[t].unsqueeze(1)
                tau = (a * (W >> 25) + ((a * (W & ((1 << 25) - 1))) >> 25)) >> (24 + log2n - 25)
                anc = torch.searchsorted(C, tau, right=True).clamp_(max=N - 1)
                x = x[(rows + anc).view(-1)]
                ll += m.squeeze(1).double() + W.squeeze(1).double().log() - const
            t += 1
    return ll


def timed(fn, reps=1):
    """Milliseconds per call of fn, by device events around `reps` calls."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs": len(ms)}


def bench_case(name, runs, reps, torch_runs):
    from viforssms_amd import _lib, ops
    model, T, K, N, chunk, dt, sd, x_true, th_true = CASES[name]
    S = len(x_true)
    obs_h, bin_h = make_data(name, T)
    obs, obs_bin = torch.as_tensor(obs_h, device=DEV), torch.as_tensor(bin_h, device=DEV)
    rng = np.random.default_rng(0)
    th = torch.as_tensor((np.asarray(th_true) + rng.uniform(-0.02, 0.02, (K, len(th_true)))).astype(np.float32),
                         device=DEV)
    x0 = torch.as_tensor(np.tile(np.asarray(x_true, np.float32), (K * N, 1)), device=DEV)
    full = ops.normal_base(SEED, 0, K * N, S * T, 0, DEV)[0].view(K * N, T, S)
    normals = [full[:, t0:t0 + chunk].permute(1, 0, 2).contiguous() for t0 in range(0, T, chunk)]
    del full
    U = torch.randint(0, 1 << 24, (T, K), device=DEV, dtype=torch.int64)
    th_rows = th.repeat_interleave(N, 0)
    fns = {"kernel": lambda: run_kernel(model, th, x0, obs, obs_bin, N, chunk, dt, sd, True),
           "nocloud": lambda: run_kernel(model, th, x0, obs, obs_bin, N, chunk, dt, sd, False)}
    tfn = lambda: run_torch(model, th_rows, x0, obs_h, bin_h, obs, normals, U, K, N, dt, sd)
    for f in fns.values():      # warm-up of every shape the timed runs use
        f()
    run_torch(model, th_rows, x0, obs_h[:, :16], bin_h[:, :16], obs, [normals[0][:16]], U, K, N, dt, sd)
    ms = {k: [] for k in fns}
    for _ in range(runs):        # alternating
        for k, f in fns.items():
            ms[k].append(timed(f, reps))
    ms["torch"] = [timed(tfn) for _ in range(torch_runs)]
    llk, lln, llt = fns["kernel"]().cpu().numpy(), fns["nocloud"]().cpu().numpy(), tfn().cpu().numpy()
    res = {"case": name, "model": model, "T": T, "K": K, "N": N, "steps_per_launch": chunk,
           "launches": (T + chunk - 1) // chunk, "observed_steps": int((bin_h != 0).any(0).sum()),
           "passes_per_timed_window": reps, "cloud_bytes": K * N * S * T * 4,
           "lds_bytes_per_block": int(_lib.load().vissm_particle_filter_lds_bytes(model, N)),
           **{k: stats(v) for k, v in ms.items()},
           "nocloud_bitwise_equal_loglik": bool(np.array_equal(llk.view(np.int64), lln.view(np.int64))),
           "kernel_loglik_mean_sd": [float(llk.mean()), float(llk.std())],
           "torch_loglik_mean_sd": [float(llt.mean()), float(llt.std())]}
    store_ms = res["kernel"]["median_ms"] - res["nocloud"]["median_ms"]
    res["cloud_store_ms"] = store_ms
    res["cloud_write_rate_bytes_per_s"] = res["cloud_bytes"] / (store_ms * 1e-3) if store_ms > 0 else None
    res["torch_over_kernel"] = res["torch"]["median_ms"] / res["kernel"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="passes over the horizon per timed window (kernels)")
    ap.add_argument("--torch-runs", type=int, default=2)
    ap.add_argument("--cases", default="ar,lv")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_filter.py needs the GPU: there is nothing to time without it")
    res = {"cases": [bench_case(c, args.runs, args.reps, args.torch_runs) for c in args.cases.split(",")]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
