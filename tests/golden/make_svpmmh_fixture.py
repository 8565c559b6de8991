"""Writes tests/golden/svpmmh_truth.npz: the theta posterior of the stochastic-volatility fixture series
(svf_series.npz: T = 64, dt = 1, h_0 = -8.5) under the prior N(PARAM_INIT, (0.05, 0.2, 0.3, 0.3)^2), from random-walk
Metropolis on the grid log-likelihood (tests/svpmmh_ref.exact_chain; 313 points of h on [-24, 2]).

The proposal factor is L = (2.38 / 2) chol(Sigma), rounded to fp32 (what the kernel takes), with Sigma put together from
a pilot's recorded numbers (64 chains x 450-600 kept draws): posterior sd (0.0036, 0.135, 0.223, 0.224), the theta_1
theta_2 correlation -0.87, every other correlation 0; the chains start at the pilot's mean (-0.0015, -0.59, -2.46,
-0.79) spread by chol(Sigma).  Then C = 128 exact chains x 1500 iterations, burn-in 300, and as many chains of the numpy
PMMH reference at N = 64 (tests/svpmmh_ref.pmmh_chain): the noise of the estimate lowers the acceptance itself, so a
PMMH run's acceptance is compared with the reference's at the same N, its mean and sd with the exact chain's.

Stored: L, prior, start; of the exact chain's kept draws the mean, the pooled sd, the standard error of the mean taken
between chains, the acceptance and its se, the split-R-hat per coordinate; ref64_{mean, sd, se, acc, acc_se} of the
reference; check_theta [256, 4] of the exact chain's kept draws and check_ll [3, 256], their log-likelihood on the
three grids of svpmmh_ref.GRID_CHECKS.  Before writing it asserts that the three grids agree to 1e-6 there and that
every split-R-hat is at most 1.05.

The chains are shared out over worker processes in blocks of 16 chains, each block on its own spawned seed, so the
result does not depend on the number of workers.  A grid evaluation of 16 chains takes 0.06 s (0.4 s for 64 chains in
one process), so one process would need tens of minutes; six workers took four (17 CPU-minutes).  It is run once.

usage: python -m tests.golden.make_svpmmh_fixture [workers]"""
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

from tests import pmmh_ref as MR
from tests import svf_ref as SR
from tests import svpmmh_ref as VR

C, N_ITER, BURN, BLOCK, REF_N = 128, 1500, 300, 16, 64
PILOT_MEAN = (-0.0015, -0.59, -2.46, -0.79)
PILOT_SD = (0.0036, 0.135, 0.223, 0.224)
PILOT_CORR12 = -0.87
SEED = 2113


def factor():
    corr = np.eye(VR.P)
    corr[1, 2] = corr[2, 1] = PILOT_CORR12
    sd = np.asarray(PILOT_SD)
    return (2.38 / np.sqrt(VR.P) * np.linalg.cholesky(corr * sd[:, None] * sd[None, :])).astype(np.float32)


def block(args):
    kind, b, th0, L, prior = args
    rng = np.random.default_rng(np.random.SeedSequence([SEED, 0 if kind == "exact" else 1, b]))
    y = VR.stat_series()
    if kind == "exact":
        r = VR.exact_chain(th0, L, prior, SR.FIX_H0, y, SR.FIX_DT, N_ITER, rng)
    else:
        r = VR.pmmh_chain(th0, L, prior, SR.FIX_H0, y, SR.FIX_DT, REF_N, N_ITER, rng)
    return r["theta"][:, BURN:], r["accept"][:, BURN:]


def main():
    workers = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    L, prior = factor(), VR.stat_prior()
    start = np.asarray(PILOT_MEAN, np.float32)
    th0 = VR.stat_start({"start": start, "L": L}, C, SEED).astype(np.float64)
    jobs = [(kind, b, th0[b * BLOCK:(b + 1) * BLOCK], L, prior) for kind in ("ref", "exact") for b in range(C // BLOCK)]
    with ProcessPoolExecutor(workers) as pool:
        res = list(pool.map(block, jobs))
    nb = C // BLOCK
    out = {"L": L, "prior": prior, "start": start}
    for kind, part in (("ref64_", res[:nb]), ("", res[nb:])):
        theta, acc = np.concatenate([p[0] for p in part]), np.concatenate([p[1] for p in part])
        s = MR.summarise(theta, acc)
        print(kind or "exact", {a: np.round(b, 4) for a, b in s.items()}, flush=True)
        out.update({f"{kind}mean": s["mean"], f"{kind}sd": s["sd"], f"{kind}se": s["se"],
                    f"{kind}acc": np.float64(s["acc"]), f"{kind}acc_se": np.float64(s["acc_se"])})
        if not kind:
            out["rhat"] = np.array([MR.split_rhat(theta[:, :, i]) for i in range(VR.P)])
            pick = np.random.default_rng(SEED).choice(theta.shape[0] * theta.shape[1], 256, replace=False)
            out["check_theta"] = theta.reshape(-1, VR.P)[pick]
    y = VR.stat_series()
    out["check_ll"] = np.stack([VR.grid_loglik_batch(out["check_theta"], SR.FIX_H0, y, SR.FIX_DT, *g)
                                for g in VR.GRID_CHECKS])
    gap = np.abs(out["check_ll"] - out["check_ll"][0]).max()
    print("rhat", out["rhat"], "grid gap", gap, flush=True)
    assert gap <= 1e-6, gap
    assert (out["rhat"] <= 1.05).all(), out["rhat"]
    np.savez(VR.FIXTURE, **out)


if __name__ == "__main__":
    main()
