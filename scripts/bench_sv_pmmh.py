"""Time the fused stochastic-volatility PMMH kernel (vissm_sv_pmmh) against the host loop a user of the SV filter could
write, by scripts/bench_pmmh.py's method.

Shapes: C = 64 and C = 256 chains of N = 1024 particles on the shipped series (dat/SV.dat, h_0 = -8.5, dt = 1) --
  sv      all T = 1508 transitions
  sv64    the first 64
Timed on each, with device events around one window of --iters iterations (sv) or --iters-short (sv64), warmed up, in
--runs alternating runs, reported per iteration:

  fused   ops.sv_pmmh: the whole window in one launch
  loop    per iteration one ops.sv_filter(cloud=False) over the whole series (one vissm_sv_filter call, h_start expanded
          once outside the window) plus torch for the proposal (randn @ L^T), the Gaussian log-prior, log(rand) and the
          decision (where), on the same tensors

Both start from the same theta (viforssms_amd.sv.PARAM_INIT jittered by 2 %) and use a factor of 1 % steps, so the
filters do the same work; their random numbers differ, so the chains agree in distribution only.  Also reported: the
filter entry alone (one ops.sv_filter(cloud=False) call for K = C, per step, from the same session), the fused kernel's
acceptance rate over the window, and the seconds of one launch of diagnostics.MCMC_LAUNCH_STEPS filter steps per block
(max(1, MCMC_LAUNCH_STEPS // T) iterations) at C = 64.

With --adaptive the adaptive kernel (ops.sv_pmmh_adaptive: the same chains, the shared factor tiled, every iteration
of the window adapting) is timed beside its twin in the same alternating runs, in place of the host loop and the filter
entry: per iteration the median and the range of both, and their ratio.

    python scripts/bench_sv_pmmh.py [--runs 5] [--iters 8] [--iters-short 100] [--adaptive] [--out FILE.json]
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

SHAPES = {"sv": None, "sv64": 64}
N, P, DT, H0 = 1024, 4, 1.0, -8.5


def setup(shape, C):
    from viforssms_amd.data import load_sv
    from viforssms_amd.sv import PARAM_INIT
    y = np.asarray(load_sv(), np.float32).reshape(-1)
    if SHAPES[shape] is not None:
        y = np.ascontiguousarray(y[:SHAPES[shape] + 1])
    rng = np.random.default_rng(0)
    th = (np.asarray(PARAM_INIT) * (1.0 + rng.uniform(-0.02, 0.02, (C, P)))).astype(np.float32)
    L = np.diag(0.01 * np.abs(np.asarray(PARAM_INIT))).astype(np.float32)
    prior = np.stack([np.zeros(P), np.full(P, 10.0)], 1).astype(np.float32)
    g = lambda a: torch.as_tensor(a, device=DEV)
    return dict(T=y.shape[0] - 1, th=g(th), L=g(L), prior=g(prior), h0=g(np.array([H0], np.float32)), y=g(y))


def filter_ll(s, th, h_rows, row0):
    from viforssms_amd import ops
    return ops.sv_filter(th, h_rows, s["y"], DT, N, SEED, row0, cloud=False).loglik


def fused(s, C, ll, n_iter):
    from viforssms_amd import ops
    return ops.sv_pmmh(s["th"], ll, s["L"], s["prior"], s["h0"], s["y"], DT, N, n_iter, SEED, C * N)


def adaptive(s, C, ll, n_iter):
    from viforssms_amd import ops
    return ops.sv_pmmh_adaptive(s["th"], ll, s["L"].repeat(C, 1, 1), s["prior"], s["h0"], s["y"], DT, N, n_iter, SEED,
                                C * N, n_iter)


def loop(s, C, ll, n_iter, h_rows):
    th, lp = s["th"], -0.5 * (((s["th"] - s["prior"][:, 0]) / s["prior"][:, 1]).double() ** 2).sum(1)
    Lt = s["L"].t().contiguous()
    for i in range(n_iter):
        prop = th + torch.randn(C, P, device=DEV) @ Lt
        lpp = -0.5 * (((prop - s["prior"][:, 0]) / s["prior"][:, 1]).double() ** 2).sum(1)
        llp = filter_ll(s, prop, h_rows, (i + 1) * C * N)
        acc = torch.rand(C, device=DEV, dtype=torch.float64).log() < (llp - ll) + (lpp - lp)
        th = torch.where(acc.unsqueeze(1), prop, th)
        ll, lp = torch.where(acc, llp, ll), torch.where(acc, lpp, lp)
    return th, ll


def bench_shape(shape, C, runs, n_iter, with_adaptive=False):
    from viforssms_amd import _lib, diagnostics
    s = setup(shape, C)
    h_rows = s["h0"].expand(C * N).contiguous()
    ll = filter_ll(s, s["th"], h_rows, 0)
    fns = {"fused": lambda: fused(s, C, ll, n_iter), "loop": lambda: loop(s, C, ll, n_iter, h_rows),
           "filter": lambda: [filter_ll(s, s["th"], h_rows, 0) for _ in range(n_iter)]}
    if with_adaptive:
        fns = {"fused": fns["fused"], "adaptive": lambda: adaptive(s, C, ll, n_iter)}
    for f in fns.values():
        f()
    ms = {k: [] for k in fns}
    for _ in range(runs):        # alternating
        for k, f in fns.items():
            ms[k].append(timed(f) / n_iter)
    r = fns["fused"]()
    T = s["T"]
    res = {"shape": shape, "T": T, "C": C, "N": N, "iterations_per_window": n_iter,
           "lds_bytes_per_block": int(_lib.load().vissm_sv_pmmh_lds_bytes(N)),
           "per_iteration": {k: stats(v) for k, v in ms.items()},
           "fused_acceptance": float(r.accept.double().mean()),
           "fused_finite_ll": bool(torch.isfinite(r.ll_chain).all())}
    med = lambda k: res["per_iteration"][k]["median_ms"]
    if with_adaptive:
        res["adaptive_over_fused"] = med("adaptive") / med("fused")
        res["adaptive_lds_bytes_per_block"] = int(_lib.load().vissm_sv_pmmh_adaptive_lds_bytes(N))
        return res
    res["loop_over_fused"] = med("loop") / med("fused")
    res["us_per_filter_step_fused"] = 1e3 * med("fused") / T
    res["us_per_filter_step_sv_filter_entry"] = 1e3 * med("filter") / T
    if C == 64:
        per = max(1, diagnostics.MCMC_LAUNCH_STEPS // T)
        res["launch"] = {"iterations": per, "seconds": timed(lambda: fused(s, C, ll, per)) * 1e-3}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=8, help="iterations per timed window at T = 1508")
    ap.add_argument("--iters-short", type=int, default=100, help="iterations per timed window at T = 64")
    ap.add_argument("--shapes", default="sv,sv64")
    ap.add_argument("--chains", default="64,256")
    ap.add_argument("--adaptive", action="store_true",
                    help="time ops.sv_pmmh_adaptive beside ops.sv_pmmh, not the host loop and the filter entry")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sv_pmmh.py needs the GPU: there is nothing to time without it")
    res = {"cases": [bench_shape(sh, int(c), args.runs, args.iters_short if sh == "sv64" else args.iters, args.adaptive)
                     for sh in args.shapes.split(",") for c in args.chains.split(",")]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
