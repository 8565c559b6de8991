"""Time the fused particle marginal Metropolis-Hastings kernel (vissm_pmmh) against the host loop a user of the adapted
filter could write.

Shapes: C = 64 and C = 256 chains of N = 1024 particles on scripts/bench_filter.py's data --
  ar      AR, T = 5000, about 70 % of the steps observed
  lv      LV, T = 1000, both species observed every 10th step
  ar64    AR, the first 64 steps of the AR series
Timed on each, with device events around one window of --iters iterations (long shapes) or --iters-short (ar64), warmed
up, in --runs alternating runs, reported per iteration:

  fused   ops.pmmh: the whole window in one launch
  loop    per iteration one ops.particle_filter(proposal="adapted", cloud=False) over the whole series (one
          vissm_particle_filter_adapted call, x_start expanded once outside the window) plus torch for the proposal
          (randn @ L^T), the Gaussian log-prior, log(rand) and the decision (where), on the same tensors

Both start from the same theta (the generator's values jittered by 2 %) and use a factor of 1 % steps, so the filters
do the same work; their random numbers differ, so the chains agree in distribution only.  Also reported: the fused
kernel's acceptance rate over the window, and the seconds of one launch of diagnostics.MCMC_LAUNCH_STEPS filter steps
per block (max(1, MCMC_LAUNCH_STEPS // T) iterations) at C = 64.

With --adaptive the adaptive kernel (ops.pmmh_adaptive: the same chains, the shared factor tiled, every iteration of
the window adapting) is timed beside its twin in the same alternating runs, in place of the host loop: per iteration
the median and the range of both, and their ratio.

    python scripts/bench_pmmh.py [--runs 5] [--iters 4] [--iters-short 100] [--adaptive] [--out FILE.json]
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

from bench_filter import CASES, DEV, SEED, make_data, stats, timed  # noqa: E402

SHAPES = {"ar": ("ar", None), "lv": ("lv", None), "ar64": ("ar", 64)}
N = 1024


def setup(shape, C):
    name, cut = SHAPES[shape]
    model, T, _, _, _, dt, sd, x_true, th_true = CASES[name]
    obs_h, bin_h = make_data(name, T)
    if cut is not None:
        obs_h, bin_h, T = np.ascontiguousarray(obs_h[:, :cut]), np.ascontiguousarray(bin_h[:, :cut]), cut
    rng = np.random.default_rng(0)
    P = len(th_true)
    th = (np.asarray(th_true) * (1.0 + rng.uniform(-0.02, 0.02, (C, P)))).astype(np.float32)
    L = np.diag(0.01 * np.abs(np.asarray(th_true))).astype(np.float32)
    prior = np.stack([np.zeros(P), np.full(P, 10.0)], 1).astype(np.float32)
    g = lambda a: torch.as_tensor(a, device=DEV)
    return dict(model=model, T=T, dt=dt, sd=sd, P=P, th=g(th), L=g(L), prior=g(prior),
                x0=g(np.asarray(x_true, np.float32)), obs=g(obs_h), obs_bin=g(bin_h),
                observed=int((bin_h != 0).any(0).sum()))


def initial_ll(s, C):
    from viforssms_amd import ops
    return ops.particle_filter(s["model"], s["th"], s["x0"], s["obs"], s["obs_bin"], s["dt"], s["sd"], N, SEED, 0,
                               cloud=False, proposal="adapted").loglik


def fused(s, C, ll, n_iter):
    from viforssms_amd import ops
    return ops.pmmh(s["model"], s["th"], ll, s["L"], s["prior"], s["x0"], s["obs"], s["obs_bin"], s["dt"], s["sd"], N,
                    n_iter, SEED, C * N)


def adaptive(s, C, ll, n_iter):
    from viforssms_amd import ops
    return ops.pmmh_adaptive(s["model"], s["th"], ll, s["L"].repeat(C, 1, 1), s["prior"], s["x0"], s["obs"],
                             s["obs_bin"], s["dt"], s["sd"], N, n_iter, SEED, C * N, n_iter)


def loop(s, C, ll, n_iter, x_rows):
    from viforssms_amd import ops
    th, lp = s["th"], -0.5 * (((s["th"] - s["prior"][:, 0]) / s["prior"][:, 1]).double() ** 2).sum(1)
    Lt = s["L"].t().contiguous()
    for i in range(n_iter):
        prop = th + torch.randn(C, s["P"], device=DEV) @ Lt
        lpp = -0.5 * (((prop - s["prior"][:, 0]) / s["prior"][:, 1]).double() ** 2).sum(1)
        llp = ops.particle_filter(s["model"], prop, x_rows, s["obs"], s["obs_bin"], s["dt"], s["sd"], N, SEED,
                                  (i + 1) * C * N, cloud=False, proposal="adapted").loglik
        acc = torch.rand(C, device=DEV, dtype=torch.float64).log() < (llp - ll) + (lpp - lp)
        th = torch.where(acc.unsqueeze(1), prop, th)
        ll, lp = torch.where(acc, llp, ll), torch.where(acc, lpp, lp)
    return th, ll


def bench_shape(shape, C, runs, n_iter, with_adaptive=False):
    from viforssms_amd import _lib, diagnostics
    s = setup(shape, C)
    ll = initial_ll(s, C)
    x_rows = s["x0"].unsqueeze(0).expand(C * N, -1).contiguous()
    fns = {"fused": lambda: fused(s, C, ll, n_iter), "loop": lambda: loop(s, C, ll, n_iter, x_rows)}
    if with_adaptive:
        fns = {"fused": fns["fused"], "adaptive": lambda: adaptive(s, C, ll, n_iter)}
    for f in fns.values():
        f()
    ms = {k: [] for k in fns}
    for _ in range(runs):        # alternating
        for k, f in fns.items():
            ms[k].append(timed(f) / n_iter)
    r = fns["fused"]()
    res = {"shape": shape, "model": s["model"], "T": s["T"], "C": C, "N": N, "observed_steps": s["observed"],
           "iterations_per_window": n_iter, "lds_bytes_per_block": int(_lib.load().vissm_pmmh_lds_bytes(s["model"], N)),
           "per_iteration": {k: stats(v) for k, v in ms.items()},
           "fused_acceptance": float(r.accept.double().mean()),
           "fused_finite_ll": bool(torch.isfinite(r.ll_chain).all())}
    if with_adaptive:
        res["adaptive_over_fused"] = (res["per_iteration"]["adaptive"]["median_ms"] /
                                      res["per_iteration"]["fused"]["median_ms"])
        res["adaptive_lds_bytes_per_block"] = int(_lib.load().vissm_pmmh_adaptive_lds_bytes(s["model"], N))
        return res
    res["loop_over_fused"] = res["per_iteration"]["loop"]["median_ms"] / res["per_iteration"]["fused"]["median_ms"]
    res["us_per_filter_step_fused"] = 1e3 * res["per_iteration"]["fused"]["median_ms"] / max(s["T"], 1)
    if C == 64:
        per = max(1, diagnostics.MCMC_LAUNCH_STEPS // s["T"])
        res["launch"] = {"iterations": per, "seconds": timed(lambda: fused(s, C, ll, per)) * 1e-3}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=4, help="iterations per timed window at the long shapes")
    ap.add_argument("--iters-short", type=int, default=100, help="iterations per timed window at ar64")
    ap.add_argument("--shapes", default="ar,lv,ar64")
    ap.add_argument("--chains", default="64,256")
    ap.add_argument("--adaptive", action="store_true", help="time ops.pmmh_adaptive beside ops.pmmh, not the host loop")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_pmmh.py needs the GPU: there is nothing to time without it")
    res = {"cases": [bench_shape(sh, int(c), args.runs, args.iters_short if sh == "ar64" else args.iters, args.adaptive)
                     for sh in args.shapes.split(",") for c in args.chains.split(",")]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
