"""Time the correlated pseudo-marginal kernel (vissm_sv_cpmmh) beside its twin (vissm_sv_pmmh), by
scripts/bench_sv_pmmh.py's method.

Shape: C = 64 chains on the shipped series (dat/SV.dat from entry 300 on, all T = 1508 transitions, h_0 = -8.5, dt = 1)
at N = 64, 256 and 1024 particles.  Timed with device events around one window of --iters iterations, warmed up, in
--runs alternating runs, reported per iteration as the median and the range:

  pmmh    ops.sv_pmmh: the ordinary chain, its filter's normals drawn in the kernel
  cpmmh   ops.sv_cpmmh at rho = 0.99 with fixed proposals (adapt_end = 0): the same chain around the sorted filter, its
          normals carried -- every step sorts the N states and moves one row of normals through memory (a 16-byte
          vector per lane and Philox group read, one written)

Both start from the same theta (viforssms_amd.sv.PARAM_INIT jittered by 2 %) and use a factor of 1 % steps.  No ratio is
demanded of the new kernel; the figures say which N to recommend.  Also reported: the acceptance of both over the
window, the bytes of carried normals per chain and the LDS per block.

    python scripts/bench_sv_cpmmh.py [--runs 5] [--iters 8] [--particles 64,256,1024] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_filter import DEV, SEED, stats, timed  # noqa: E402
from bench_sv_pmmh import DT, setup  # noqa: E402

C, RHO = 64, 0.99


def bench_n(s, N, runs, n_iter):
    from viforssms_amd import _lib, ops
    T = s["T"]
    ll = ops.sv_filter(s["th"], s["h0"], s["y"], DT, N, SEED, 0, cloud=False).loglik
    aux = ops.cpm_fresh_aux(C, T, N, SEED ^ 0x5A5A, 0, DEV)
    ll_c = ops.sv_filter_sorted(s["th"], s["h0"], s["y"], DT, N, aux[0][:, 0].contiguous(),
                                aux[1][:, 0].contiguous()).loglik
    chol = s["L"].repeat(C, 1, 1)
    # the timed launches go on mutating these; ll_c no longer goes with them, which timing does not mind
    work = [a.clone() for a in aux]
    fns = {"pmmh": lambda: ops.sv_pmmh(s["th"], ll, s["L"], s["prior"], s["h0"], s["y"], DT, N, n_iter, SEED, C * N),
           "cpmmh": lambda: ops.sv_cpmmh(s["th"], ll_c, chol, s["prior"], s["h0"], s["y"], DT, N, n_iter, SEED, C * N, RHO,
                                         *work)}
    for f in fns.values():
        f()
    ms = {k: [] for k in fns}
    for _ in range(runs):        # alternating
        for k, f in fns.items():
            ms[k].append(timed(f) / n_iter)
    for a, w in zip(aux, work):          # the acceptance from the state ll_c belongs to
        w.copy_(a)
    acc = {k: float(f().accept.double().mean()) for k, f in fns.items()}
    res = {"T": T, "C": C, "N": N, "rho": RHO, "iterations_per_window": n_iter,
           "per_iteration": {k: stats(v) for k, v in ms.items()}, "acceptance": acc,
           "aux_bytes_per_chain": int(aux[0][0].numel() + aux[1][0].numel()) * 4,
           "lds_bytes_per_block": {"pmmh": int(_lib.load().vissm_sv_pmmh_lds_bytes(N)),
                                   "cpmmh": int(_lib.load().vissm_sv_cpmmh_lds_bytes(N))}}
    med = lambda k: res["per_iteration"][k]["median_ms"]
    res["cpmmh_over_pmmh"] = med("cpmmh") / med("pmmh")
    res["us_per_filter_step"] = {k: 1e3 * med(k) / T for k in fns}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=8, help="iterations per timed window")
    ap.add_argument("--particles", default="64,256,1024")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sv_cpmmh.py needs the GPU: there is nothing to time without it")
    s = setup("sv", C)
    res = {"cases": [bench_n(s, int(n), args.runs, args.iters) for n in args.particles.split(",")]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
