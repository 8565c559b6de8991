"""Writes tests/golden/pmmh_ar_truth.npz: the theta posterior of the AR fixture series (pf_ar_series.npz, x0 = 10,
obs_std = 1) from random-walk Metropolis on the exact Kalman log-likelihood (tests/pmmh_ref.exact_chain), under two
priors: "flat", (0, 10) on every coordinate, and "informative", N(5, 0.5^2) on theta_0 -- a chain that drops the prior
passes the first and fails the second.

Per case: a pilot of 256 chains x 1000 iterations from the generator's theta with a diagonal proposal; L = chol(2.38^2 /
3 * the pilot's second-half covariance), rounded to fp32 (what the kernel takes); then 256 chains x 1500 iterations from
the pilot's mean, burn-in 300.  Stored: L, prior, start, and of the kept draws the mean, the pooled sd, the standard
error of the mean taken between chains, and the acceptance rate.

usage: python -m tests.golden.make_pmmh_fixture"""
import numpy as np

from tests import pf_ref as PR
from tests import pmmh_ref as MR
from tests import sim_util as SU

C, N_ITER, BURN = 256, 1500, 300
PRIORS = {"flat": [(0.0, 10.0)] * 3, "informative": [(5.0, 0.5), (0.0, 10.0), (0.0, 10.0)]}


def main():
    obs, obs_bin = PR.stat_case()
    out = {}
    for k, (case, prior) in enumerate(PRIORS.items()):
        prior = np.asarray(prior, np.float32)
        rng = np.random.default_rng(20 + k)
        th0 = np.tile(np.asarray(SU.TRUE_THETA[SU.AR]), (C, 1))
        pilot = MR.exact_chain(th0, np.diag([0.5, 0.05, 0.05]), prior, MR.STAT_X0, obs, obs_bin, MR.STAT_OBS_STD, 1000,
                               rng)["theta"][:, 500:].reshape(-1, 3)
        L = np.linalg.cholesky(2.38 ** 2 / 3.0 * np.cov(pilot.T)).astype(np.float32)
        start = pilot.mean(0).astype(np.float32)
        r = MR.exact_chain(np.tile(start.astype(np.float64), (C, 1)), L, prior, MR.STAT_X0, obs, obs_bin,
                           MR.STAT_OBS_STD, N_ITER, rng)
        s = MR.summarise(r["theta"][:, BURN:], r["accept"][:, BURN:])
        print(case, {a: np.round(b, 4) for a, b in s.items()})
        out.update({f"{case}_L": L, f"{case}_prior": prior, f"{case}_start": start, f"{case}_mean": s["mean"],
                    f"{case}_sd": s["sd"], f"{case}_se": s["se"], f"{case}_acc": np.float64(s["acc"]),
                    f"{case}_acc_se": np.float64(s["acc_se"])})
    np.savez(MR.FIXTURE, **out)


if __name__ == "__main__":
    main()
