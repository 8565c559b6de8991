"""Time the fully adapted particle filter (vissm_particle_filter_adapted) beside the bootstrap filter on the same data,
and measure what it buys: the spread of the log-evidence estimate.

The shapes, data, launches per horizon and timing method are scripts/bench_filter.py's (AR T = 5000 and LV T = 1000,
K = 64 filters of N = 1024 particles; device events around --reps back-to-back passes over the whole horizon, warmed
up, --runs alternating runs, median and range).  Timed per shape, with the cloud written and with cloud = NULL:

  bootstrap  ops.particle_filter(proposal="bootstrap") of this build
  adapted    ops.particle_filter(proposal="adapted")
  parent     with --parent-lib PATH: vissm_particle_filter of another build of libvissm.so (the parent commit's), called
             through ctypes on the same tensors -- the bootstrap kernel as it was before the proposal parameter

Then, at one common theta (the generators' true values for all K filters, so the spread is the estimator's own), the
mean and sd of loglik over the K filters for both proposals, and sd^2 x time: the compute a given precision costs.

    python scripts/bench_filter_adapted.py [--runs 5] [--reps 3] [--parent-lib PATH] [--out FILE.json]
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_filter import CASES, DEV, SEED, make_data, stats, timed  # noqa: E402


def run_ops(proposal, model, th, x0, obs, obs_bin, N, chunk, dt, sd, cloud):
    from viforssms_amd import ops
    T = obs.shape[1]
    state, ll = x0, None
    for t0 in range(0, T, chunk):
        r = ops.particle_filter(model, th, state, obs, obs_bin, dt, sd, N, SEED, 0, t0=t0, loglik_in=ll, cloud=cloud,
                                H=min(chunk, T - t0), proposal=proposal)
        state, ll = r.state_end, r.loglik
    return ll


def parent_runner(path):
    """run(...) with run_ops' arguments that calls vissm_particle_filter of the library at `path` directly."""
    from viforssms_amd import _lib
    lib = ctypes.CDLL(path)
    fn = lib.vissm_particle_filter
    fn.restype, fn.argtypes = _lib.SIGNATURES["vissm_particle_filter"]
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def run(model, th, x0, obs, obs_bin, N, chunk, dt, sd, cloud):
        K, S, T = th.shape[0], x0.shape[1], obs.shape[1]
        state, ll = x0, None
        for t0 in range(0, T, chunk):
            H = min(chunk, T - t0)
            out = torch.empty(K, dtype=torch.float64, device=DEV)
            inc, ess = torch.empty(K, H, device=DEV), torch.empty(K, H, device=DEV)
            end = torch.empty(K * N, S, device=DEV)
            cl = torch.empty(K * N, S, H, device=DEV) if cloud else None
            d = _lib.PfDesc(model, K, N, H, t0, T, float(dt), float(sd))
            rc = fn(ctypes.byref(d), SEED, 0, p(th), p(state), p(obs), p(obs_bin), p(ll), p(out), p(inc), p(ess),
                    p(end), p(cl), None, None, _lib.stream_handle(torch.device(DEV)))
            assert rc == 0, rc
            state, ll = end, out
        return ll
    return run


def bench_case(name, runs, reps, parent):
    from viforssms_amd import _lib
    model, T, K, N, chunk, dt, sd, x_true, th_true = CASES[name]
    S = len(x_true)
    obs_h, bin_h = make_data(name, T)
    obs, obs_bin = torch.as_tensor(obs_h, device=DEV), torch.as_tensor(bin_h, device=DEV)
    rng = np.random.default_rng(0)
    th = torch.as_tensor((np.asarray(th_true) + rng.uniform(-0.02, 0.02, (K, len(th_true)))).astype(np.float32),
                         device=DEV)
    th_one = torch.as_tensor(np.tile(np.asarray(th_true, np.float32), (K, 1)), device=DEV)
    x0 = torch.as_tensor(np.tile(np.asarray(x_true, np.float32), (K * N, 1)), device=DEV)
    args = (model, th, x0, obs, obs_bin, N, chunk, dt, sd)
    fns = {}
    for cloud, tag in ((True, ""), (False, "_nocloud")):
        fns["bootstrap" + tag] = lambda c=cloud: run_ops("bootstrap", *args, c)
        fns["adapted" + tag] = lambda c=cloud: run_ops("adapted", *args, c)
        if parent is not None:
            fns["parent" + tag] = lambda c=cloud: parent(*args, c)
    for f in fns.values():
        f()
    ms = {k: [] for k in fns}
    for _ in range(runs):        # alternating
        for k, f in fns.items():
            ms[k].append(timed(f, reps))
    res = {"case": name, "model": model, "T": T, "K": K, "N": N, "steps_per_launch": chunk,
           "observed_steps": int((bin_h != 0).any(0).sum()), "obs_std": sd, "passes_per_timed_window": reps,
           "lds_bytes_per_block": int(_lib.load().vissm_particle_filter_adapted_lds_bytes(model, N)),
           **{k: stats(v) for k, v in ms.items()}}
    res["adapted_over_bootstrap"] = res["adapted"]["median_ms"] / res["bootstrap"]["median_ms"]
    res["adapted_over_bootstrap_nocloud"] = res["adapted_nocloud"]["median_ms"] / res["bootstrap_nocloud"]["median_ms"]
    if parent is not None:
        res["bootstrap_over_parent"] = res["bootstrap"]["median_ms"] / res["parent"]["median_ms"]
        a, b = fns["parent"]().cpu().numpy(), fns["bootstrap"]().cpu().numpy()
        res["bootstrap_bitwise_equals_parent"] = bool(np.array_equal(a.view(np.int64), b.view(np.int64)))
    one = (model, th_one, x0, obs, obs_bin, N, chunk, dt, sd, False)
    for prop in ("bootstrap", "adapted"):
        ll = run_ops(prop, *one).cpu().numpy()
        fin = ll[np.isfinite(ll)]
        res[f"{prop}_common_theta"] = {"finite": int(fin.size), "mean": float(fin.mean()), "sd": float(fin.std(ddof=1))}
        res[f"{prop}_sd2_x_ms"] = float(fin.std(ddof=1)) ** 2 * res[f"{prop}_nocloud"]["median_ms"]
    res["sd_ratio_adapted_over_bootstrap"] = res["adapted_common_theta"]["sd"] / res["bootstrap_common_theta"]["sd"]
    res["sd2_x_ms_ratio_bootstrap_over_adapted"] = res["bootstrap_sd2_x_ms"] / res["adapted_sd2_x_ms"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="passes over the horizon per timed window")
    ap.add_argument("--cases", default="ar,lv")
    ap.add_argument("--parent-lib", default=None, help="a libvissm.so of the parent commit to time beside this build")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_filter_adapted.py needs the GPU: there is nothing to time without it")
    parent = parent_runner(args.parent_lib) if args.parent_lib else None
    res = {"parent_lib": bool(parent), "cases": [bench_case(c, args.runs, args.reps, parent)
                                                  for c in args.cases.split(",")]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
