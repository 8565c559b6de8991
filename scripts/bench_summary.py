"""Time the posterior summary of one window at the AR configuration shape against a torch baseline.

x [B, M + 1] fp32 (65536 x 5001 by default) is drawn once from the AR model's forward (random-init weights, the
benchmark's data: bench.py build_model).  Timed on it, with device events, warmed up, in alternating runs:

  summary   summary.column_summary(x, probs): vissm_col_moments + the 4-pass radix select + the host interpolation,
            up to and including the copy of the few KB of results
  torch     the same statistics from torch.sort(x, dim=0): the rows of the sorted matrix at the same ranks, the
            linear interpolation, mean and std, copied to the host

and, in a run of their own, the summary's phases (moments, each byte's histograms, the narrowing steps).  Reported:
both times per run, the peak extra device memory of each (torch.cuda.max_memory_allocated deltas), the two results'
agreement, and the summary's time against its byte floor: passes over x (1 for the moments + 4 for the select)
x B x n_cols x 4 bytes / 8 TB/s -- derived from the shape and the HBM peak, not measured.

    python scripts/bench_summary.py [--B 65536] [--M 5000] [--runs 3] [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12   # bytes / s (MI355X)


def build_x(B, M, k, precision):
    """One window's paths [B, M + 1] from the AR model's forward (bench.py's AR model and data)."""
    from viforssms_amd import _lib
    from viforssms_amd.ar import VI_SSM, build_theta_spec
    from viforssms_amd.data import data_gen
    np.random.seed(1)
    np.random.seed(1)
    obs, ob, tt = data_gen(M, 5, 10.0, np.array([5.0, 0.5, 3.0]), 1.0, write=False)
    obs, ob, tt = (np.asarray(a, dtype=np.float32) for a in (obs, ob, tt))
    spec = build_theta_spec([(0.0, 10.0)] * 3)
    model = VI_SSM(obs, 1.0, 10.0, spec, [(0.0, 10.0)] * 3, M, B, k, M, [50, 50, 50], 3, 10, ob, tt, pre_train=False,
                   device="cuda:0", precision=_lib.TRAIN_PRECISIONS[precision], log_every=10 ** 9)
    x = model.sample_paths(np.tile(0, B), step=0)
    x = x[:, 0, :].contiguous()
    del model
    torch.cuda.empty_cache()
    return x


def timed(fn):
    """(result, milliseconds by device events, peak extra device bytes) of fn(); fn ends with a host copy."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    res = fn()
    e1.record()
    torch.cuda.synchronize()
    return res, e0.elapsed_time(e1), torch.cuda.max_memory_allocated() - base


def torch_baseline(x, probs):
    B = x.shape[0]
    srt = torch.sort(x, dim=0).values
    pos = (B - 1) * np.asarray(probs, dtype=np.float64)
    lo, hi = np.floor(pos).astype(np.int64), np.ceil(pos).astype(np.int64)
    t = torch.as_tensor(pos - lo, device=x.device).unsqueeze(1)
    a, b = srt[torch.as_tensor(lo, device=x.device)].double(), srt[torch.as_tensor(hi, device=x.device)].double()
    q = a + (b - a) * t
    xd_mean = x.mean(0, dtype=torch.float64)
    sd = x.std(0, unbiased=False)
    return {"quantiles": q.cpu().numpy(), "mean": xd_mean.cpu().numpy(), "sd": sd.double().cpu().numpy()}


def phases(x, probs):
    """Milliseconds of the summary's device phases (one run, device events around each C-ABI call)."""
    from viforssms_amd import _lib, ops
    lib = _lib.load()
    dev = x.device
    B, n = x.shape
    n_ranks = 2 * len(probs)
    d = _lib.ColStatDesc(B, n, x.stride(0), n_ranks)
    pos = (B - 1) * np.asarray(probs, dtype=np.float64)          # the ranks column_summary asks for
    ranks = torch.as_tensor(np.concatenate([np.floor(pos), np.ceil(pos)]).astype(np.int32), device=dev)
    rank_left = ranks.expand(n, n_ranks).contiguous()
    prefix = torch.empty(n, n_ranks, dtype=torch.int32, device=dev)
    hist = torch.empty(n, n_ranks, 256, dtype=torch.int32, device=dev)
    st = _lib.stream_handle(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(10)]
    ops.col_moments(x)
    torch.cuda.synchronize()
    ev[0].record()
    ops.col_moments(x)
    ev[1].record()
    for p in range(4):
        _lib.check(lib.vissm_col_select_hist(ctypes.byref(d), x.data_ptr(), prefix.data_ptr(), p, hist.data_ptr(), None,
                                             st), "hist")
        ev[2 + 2 * p].record()
        _lib.check(lib.vissm_col_select_narrow(ctypes.byref(d), hist.data_ptr(), rank_left.data_ptr(),
                                               prefix.data_ptr(), p, st), "narrow")
        ev[3 + 2 * p].record()
    torch.cuda.synchronize()
    out = {"moments_ms": ev[0].elapsed_time(ev[1])}
    for p in range(4):
        out[f"hist{p}_ms"] = ev[1 + 2 * p].elapsed_time(ev[2 + 2 * p])
        out[f"narrow{p}_ms"] = ev[2 + 2 * p].elapsed_time(ev[3 + 2 * p])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--M", type=int, default=5000)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_summary.py needs the GPU: there is nothing to time without it")
    from viforssms_amd.summary import DEFAULT_PROBS, column_summary

    x = build_x(args.B, args.M, args.k, args.precision)
    B, n = x.shape
    probs = DEFAULT_PROBS
    run_summary = lambda: column_summary(x, probs)
    run_torch = lambda: torch_baseline(x, probs)
    s, _, _ = timed(run_summary)      # warm-up of every shape the timed runs use
    t, _, _ = timed(run_torch)
    runs = []
    for _ in range(args.runs):         # alternating
        _, ms_s, mem_s = timed(run_summary)
        _, ms_t, mem_t = timed(run_torch)
        runs.append({"summary_ms": ms_s, "torch_ms": ms_t, "summary_peak_bytes": mem_s, "torch_peak_bytes": mem_t})
    ph = phases(x, probs)
    passes = 5
    floor_ms = passes * B * n * 4 / HBM_PEAK * 1e3
    best = min(r["summary_ms"] for r in runs)
    finite = np.isfinite(t["quantiles"]) & np.isfinite(s["quantiles"])
    res = {
        "shape": [B, n], "probs": list(probs), "runs": runs, "phases": ph,
        "summary_faster_in_every_pair": all(r["summary_ms"] < r["torch_ms"] for r in runs),
        "x_bytes": B * n * 4,
        "hist_bytes": n * 2 * len(probs) * 1024,
        "byte_floor_ms": floor_ms, "byte_floor_passes": passes,
        "floor_over_best_summary": floor_ms / best,
        "quantiles_max_rel_diff_vs_torch": float(np.max(np.abs(s["quantiles"] - t["quantiles"])[finite]
                                                        / np.maximum(np.abs(t["quantiles"])[finite], 1e-300)))
        if finite.any() else None,
        "x_abs_max": float(x.abs().max()), "x_nonfinite": int((~torch.isfinite(x)).sum()),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
