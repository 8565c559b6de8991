"""Time the forecast kernel (vissm_sde_simulate) against a torch restatement of the same Euler-Maruyama chains.

Two shapes, the horizon cut into launches as VISSMBase.forecast cuts it (chained through x_end and t0):

  AR   B = 65536, H = 5000   (1024 steps per launch: the forecast's default byte budget)
  LV   B = 16384, H = 1000   (one launch)

Timed on each, with device events around --reps back-to-back passes over the whole horizon (one pass is under a
millisecond: too short a window on its own), warmed up, in alternating runs, reported per pass:

  kernel   the production library's vissm_sde_simulate: normals drawn in the kernel, tiles staged in LDS
  direct   (--variant-lib) a build of the same unit with -DVISSM_SIM_DIRECT_STORE (make SIM_EXTRA=...): every lane
           stores its own row, no staging -- the A/B of the store path, loaded next to the production library
  torch    the parent has no such kernel, so the yardstick is the same step per model as a loop over t on [B, S]
           tensors, the normals pre-drawn by ops.normal_base outside the timed window, the dead-row rule included

Reported per shape: median, minimum and maximum milliseconds of each over --runs runs, the bytes the kernel writes
(B S H 4, x only) over its median time against the 8 TB/s HBM peak, whether kernel and direct agree bitwise, and the
largest |kernel - torch| over the finite entries (they share the normals; the arithmetic differs in contraction).

    python scripts/bench_forecast.py [--runs 5] [--reps 20] [--variant-lib PATH] [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12   # bytes / s (MI355X)
DEV = "cuda:0"
SEED = 1234
# model id, B, H, steps per launch, dt, start state, raw theta (the generators' true values)
CASES = {"ar": (0, 65536, 5000, 1024, 1.0, [10.0], [5.0, 0.5, float(np.log(3.0))]),
         "lv": (1, 16384, 1000, 1000, 0.1, [100.0, 100.0], [float(v) for v in np.log([0.5, 0.0025, 0.3])])}


def load_variant(path):
    from viforssms_amd import _lib
    lib = ctypes.CDLL(path)
    res, args = _lib.SIGNATURES["vissm_sde_simulate"]
    lib.vissm_sde_simulate.restype, lib.vissm_sde_simulate.argtypes = res, args
    return lib


def run_kernel(lib, model, th, x0, H, chunk, dt, keep=False):
    """The whole horizon through `lib`, chunk steps per launch into one reused buffer; returns the last chunk's
    x (or every chunk's, keep=True) and x_end."""
    from viforssms_amd import _lib
    B, S = x0.shape
    st = _lib.stream_handle(th.device)
    buf = torch.empty(B * S * min(chunk, H), dtype=torch.float32, device=th.device)
    state, nxt = x0.clone(), torch.empty_like(x0)
    kept = []
    for t0 in range(0, H, chunk):
        m = min(chunk, H - t0)
        d = _lib.SimDesc(model, B, m, t0, S, dt, 0.0, 0)
        rc = lib.vissm_sde_simulate(ctypes.byref(d), SEED, 0, th.data_ptr(), state.data_ptr(), buf.data_ptr(), None,
                                    nxt.data_ptr(), st)
        assert rc == 0, rc
        state, nxt = nxt, state
        if keep:
            kept.append(buf[:B * S * m].view(B, S, m).clone())
    return (torch.cat(kept, 2) if keep else buf), state


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


def run_torch(model, th, x0, normals, chunk, dt, keep=False):
    """The restatement over the pre-drawn normals (a list of time-major [m, B, S] tensors, one per launch of the
    kernel)."""
    B, S = x0.shape
    x = x0.clone()
    buf = torch.empty(B, S, chunk, dtype=torch.float32, device=th.device)
    kept = []
    for nn in normals:
        m = nn.shape[0]
        for t in range(m):
            x = torch_step(model, x, th, dt, nn[t])
            buf[:, :, t] = x
        if keep:
            kept.append(buf[:, :, :m].clone())
    return (torch.cat(kept, 2) if keep else buf), x


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


def bench_case(name, runs, reps, torch_runs, variant):
    from viforssms_amd import _lib, ops
    model, B, H, chunk, dt, x_true, th_true = CASES[name]
    S = len(x_true)
    lib = _lib.load()
    rng = np.random.default_rng(0)
    th = torch.as_tensor((np.asarray(th_true) + rng.uniform(-0.05, 0.05, (B, len(th_true)))).astype(np.float32),
                         device=DEV)
    x0 = torch.as_tensor((np.asarray(x_true) * rng.uniform(0.95, 1.05, (B, S))).astype(np.float32), device=DEV)
    # the numbers the kernel consumes: entry (t0 + t) S + i of row b; time-major copies for the step loop
    full = ops.normal_base(SEED, 0, B, S * H, 0, DEV)[0].view(B, H, S)
    normals = [full[:, t0:t0 + chunk].permute(1, 0, 2).contiguous() for t0 in range(0, H, chunk)]
    del full
    fns = {"kernel": lambda: run_kernel(lib, model, th, x0, H, chunk, dt)}
    if variant is not None:
        fns["direct"] = lambda: run_kernel(variant, model, th, x0, H, chunk, dt)
    for f in fns.values():      # warm-up of every shape the timed runs use
        f()
    run_torch(model, th, x0, [normals[0][:8]], chunk, dt)
    ms = {k: [] for k in fns}
    for _ in range(runs):        # alternating
        for k, f in fns.items():
            ms[k].append(timed(f, reps))
    ms["torch"] = [timed(lambda: run_torch(model, th, x0, normals, chunk, dt)) for _ in range(torch_runs)]
    # agreement, on the first launch's steps
    m = min(chunk, H, 256)
    xk, _ = run_kernel(lib, model, th, x0, m, m, dt, keep=True)
    xt, _ = run_torch(model, th, x0, [normals[0][:m]], m, dt, keep=True)
    fin = torch.isfinite(xk) & torch.isfinite(xt)
    res = {"case": name, "model": model, "B": B, "H": H, "steps_per_launch": chunk,
           "launches": (H + chunk - 1) // chunk, "passes_per_timed_window": reps,
           "x_bytes": B * S * H * 4,
           **{k: stats(v) for k, v in ms.items()},
           "kernel_vs_torch_max_abs_diff_first_steps": float((xk - xt)[fin].abs().max()),
           "kernel_nan_share_first_steps": float(torch.isnan(xk).float().mean())}
    res["kernel_write_rate_bytes_per_s"] = res["x_bytes"] / (res["kernel"]["median_ms"] * 1e-3)
    res["kernel_share_of_hbm_peak"] = res["kernel_write_rate_bytes_per_s"] / HBM_PEAK
    res["torch_over_kernel"] = res["torch"]["median_ms"] / res["kernel"]["median_ms"]
    if variant is not None:
        xd, _ = run_kernel(variant, model, th, x0, m, m, dt, keep=True)
        res["direct_bitwise_equal_first_steps"] = bool(torch.equal(xk.view(torch.int32), xd.view(torch.int32)))
        res["direct_over_kernel"] = res["direct"]["median_ms"] / res["kernel"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20, help="passes over the horizon per timed window (kernels)")
    ap.add_argument("--torch-runs", type=int, default=2)
    ap.add_argument("--cases", default="ar,lv")
    ap.add_argument("--variant-lib", default=None, help="a -DVISSM_SIM_DIRECT_STORE build of libvissm.so")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_forecast.py needs the GPU: there is nothing to time without it")
    variant = load_variant(args.variant_lib) if args.variant_lib else None
    res = {"cases": [bench_case(c, args.runs, args.reps, args.torch_runs, variant) for c in args.cases.split(",")],
           "variant_lib": bool(variant)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
