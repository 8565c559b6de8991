"""hyperparameters.txt format and the main.py command line (main.py:6-57, 59-130 of the reference).

The file is read positionally: values sit at 0-based line indices 1, 3, ..., 27 in the order
T, impute, x0, theta, obs_std, p, kernel_len, batch_dims, network_dims, no_flows, priors,
feat_window, learn_rate, grad_clip.  Command-line overrides win over the file.  Extra flags of
this build (not in the reference): -p/-samples, --gpus, --steps, --seed, --precision, --no-pretrain.
"""
from __future__ import annotations

import argparse
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

DEFAULT_FILE = """#### T ####
5000
#### impute ####
1
#### x0 ####
10.0
#### Theta ####
5.0, 0.5, 3.0
#### Observation Standard Deviation ####
1.
#### p ####
50
#### kernel_len ####
50
#### batch_dims ####
50
#### network_dims ####
50, 50, 50
#### no_flows ####
3
####  priors ####
(0., 10.0)(0., 10.0)(0., 10.0)
#### feat_window ####
10
#### learn_rate ####
1e-3
#### grad_clip ####
2.5e8
"""


@dataclass
class HyperParams:
    T: int
    impute: int
    x0: float
    theta: List[float]
    obs_std: float
    p: int
    kernel_len: int
    batch_dims: int
    network_dims: List[int]
    no_flows: int
    priors: List[Tuple[float, float]]
    feat_window: int
    learn_rate: float
    grad_clip: float


def parse_priors(line: str) -> List[Tuple[float, float]]:
    parts = line.rstrip().replace(")", "").split("(")[1:]
    return [(float(t.split(",")[0]), float(t.split(",")[1])) for t in parts]


def parseparams(file) -> list:
    """Positional parse (reference main.py:26-57); returns the 14 values as a list."""
    with open(file, "r") as f:
        lines = f.readlines()
    vals = [
        int(lines[1].rstrip()),
        int(lines[3].rstrip()),
        float(lines[5].rstrip()),
        [float(t) for t in lines[7].rstrip().split(",")],
        float(lines[9].rstrip()),
        int(lines[11].rstrip()),
        int(lines[13].rstrip()),
        int(lines[15].rstrip()),
        [int(d) for d in lines[17].rstrip().split(",")],
        int(lines[19].rstrip()),
        parse_priors(lines[21]),
        int(lines[23].rstrip()),
        float(lines[25].rstrip()),
        float(lines[27].rstrip()),
    ]
    return vals


def to_hparams(vals: list) -> HyperParams:
    return HyperParams(*vals)


def handle_opts(argv=None):
    parser = argparse.ArgumentParser(
        formatter_class=argparse.RawDescriptionHelpFormatter,
        description="Neural moving-average variational inference for SDEs on MI355X (AR(1) driver).",
        usage="%(prog)s hyperparameters.txt [OPTIONS] \n Any options passed will be prioritised over the setting "
              "in the hyperparameters text file. \n To repair your hyperparameters file use -repair and copy and "
              "paste the output into hyperparameters.txt")
    parser.add_argument("file", action="store", nargs="?", default=None, help="File containing all hyperparameters")
    parser.add_argument("-T", "-time", action="store", dest="T", default=None, help="Time")
    parser.add_argument("-i", "-impute", action="store", dest="impute", default=None, help="Impute")
    parser.add_argument("-t", "-theta", action="append", dest="theta", default=None, help="Theta values listed")
    parser.add_argument("-x", "-xzero", action="store", dest="x0", default=None, help="Value for x at time 0")
    parser.add_argument("-o", "-obs_std", action="store", dest="obs_std", default=None,
                        help="Observation standard deviation")
    parser.add_argument("-k", "-kernel_len", action="store", dest="kernel_len", default=None, help="Length of Kernel")
    parser.add_argument("-b", "-batch_dims", action="store", dest="batch_dims", default=None,
                        help="Batch Dimensions (window length M)")
    parser.add_argument("-f", "-feat_window", action="store", dest="feat_window", default=None, help="Feature Window")
    parser.add_argument("-repair", action="store_true", dest="repair", default=False,
                        help="Output default hyperparameters to repair file")
    # additions of this build
    parser.add_argument("-p", "-samples", action="store", dest="p", default=None,
                        help="Samples (windows) per step; overrides the file's p")
    parser.add_argument("--gpus", type=int, default=None,
                        help="Ranks (one per GPU): without torchrun, N > 1 launches N ranks itself; under torchrun "
                             "the launched world must equal N.  Default: the launcher's world (1 without one)")
    parser.add_argument("--steps", type=int, default=None, help="Stop after this many runs (default: endless)")
    parser.add_argument("--seed", type=int, default=1, help="Philox seed of the base noise")
    parser.add_argument("--precision", choices=["fp32", "bf16", "bf16x2", "bf16x3", "bf16x3f", "bf16x2f"],
                        default="fp32",
                        help="flow products: fp32 exact, bf16, bf16x2 (split weights, bf16 activations, forward and "
                             "backward), bf16x3 (split operands); bf16x3f / bf16x2f: "
                             "bf16x3 / split-weight forward products with bf16 backward products")
    parser.add_argument("--no-pretrain", action="store_true", help="Skip the 501 pre-training runs")
    parser.add_argument("--log-every", type=int, default=1)
    parser.add_argument("--graph", action="store_true",
                        help="Run the ELBO steps as a captured HIP graph (launch-bound small configs)")
    parser.add_argument("--summary", metavar="PATH", default=None,
                        help="After training, write the posterior summary (mean, sd and quantile bands of the latent "
                             "path over time and of theta, computed on the GPU) to this .npz file")
    parser.add_argument("--forecast", nargs=2, metavar=("H", "PATH"), default=None,
                        help="After training, simulate the fitted model H steps past the data on the GPU and write the "
                             "posterior-predictive forecast (mean, sd and quantile bands over time) to this .npz file")
    parser.add_argument("--filter", nargs=3, metavar=("K", "N", "PATH"), default=None,
                        help="After training, run K bootstrap particle filters of N particles each (64 .. 1024, a "
                             "power of two) on the GPU, one per posterior theta sample, and write their log-evidence "
                             "estimates and filtering bands to this .npz file")
    parser.add_argument("--smooth", nargs=4, metavar=("K", "N", "M", "PATH"), default=None,
                        help="After training, run the K particle filters of N particles of --filter and then draw M "
                             "smoothing trajectories per filter by backward simulation on the GPU (M a power of two, "
                             "64 <= M <= N), and write the filter's entries and the smoothing bands to this .npz file")
    parser.add_argument("--filter-proposal", choices=("bootstrap", "adapted"), default=None,
                        help="The proposal of the particle filters of --filter and --smooth: bootstrap (the default) "
                             "propagates blindly and weights on the observation; adapted weights on the predictive "
                             "p(y_t | x_t-1) and propagates from p(x_t | x_t-1, y_t), a much lower variance of the "
                             "log-evidence where obs_std is small against the process noise")
    parser.add_argument("--mcmc", nargs=4, metavar=("C", "N", "ITER", "PATH"), default=None,
                        help="After training, run C particle marginal Metropolis-Hastings chains of ITER iterations on "
                             "the GPU, each with a fully adapted particle filter of N particles (64 .. 1024, a power of "
                             "two), started at posterior theta samples, and write the draws of p(theta | y) after the "
                             "default burn-in, their quantiles beside q(theta)'s and the split-R-hat to this .npz file")
    parser.add_argument("--mcmc-adapt", action="store_true",
                        help="With --mcmc: every chain adapts its own proposal on the GPU over the first half of the "
                             "iterations (robust adaptive Metropolis towards 23.4 %% acceptance) and keeps it frozen "
                             "over the second half, which is kept; for a q(theta) much wider than the posterior, where "
                             "the shared proposal accepts a few per mille.  Also written: the chains' final factors "
                             "and their acceptance while adapting")
    args = parser.parse_args(argv)
    if args.mcmc_adapt and args.mcmc is None:
        parser.error("--mcmc-adapt applies to --mcmc: give it")
    if args.mcmc is not None:
        try:
            args.mcmc = (int(args.mcmc[0]), int(args.mcmc[1]), int(args.mcmc[2]), args.mcmc[3])
        except ValueError:
            parser.error(f"--mcmc: C, N and ITER must be integers, got {args.mcmc[:3]!r}")
        if args.mcmc[0] < 1 or args.mcmc[1] not in (64, 128, 256, 512, 1024) or args.mcmc[2] < 2:
            parser.error("--mcmc: C >= 1, N one of 64, 128, 256, 512, 1024 and ITER >= 2 expected")
    if args.filter_proposal is not None and args.filter is None and args.smooth is None:
        parser.error("--filter-proposal applies to --filter and --smooth: give one of them")
    if args.filter_proposal is None:
        args.filter_proposal = "bootstrap"
    if args.smooth is not None:
        try:
            args.smooth = (int(args.smooth[0]), int(args.smooth[1]), int(args.smooth[2]), args.smooth[3])
        except ValueError:
            parser.error(f"--smooth: K, N and M must be integers, got {args.smooth[:3]!r}")
        k_, n_, m_ = args.smooth[:3]
        if k_ < 1 or n_ not in (64, 128, 256, 512, 1024) or not (64 <= m_ <= n_ and m_ & (m_ - 1) == 0):
            parser.error("--smooth: K >= 1, N one of 64, 128, 256, 512, 1024 and M a power of two in 64 .. N expected")
    if args.filter is not None:
        try:
            args.filter = (int(args.filter[0]), int(args.filter[1]), args.filter[2])
        except ValueError:
            parser.error(f"--filter: K and N must be integers, got {args.filter[0]!r} {args.filter[1]!r}")
        if args.filter[0] < 1 or args.filter[1] not in (64, 128, 256, 512, 1024):
            parser.error("--filter: K >= 1 and N one of 64, 128, 256, 512, 1024 expected")
    if args.forecast is not None:
        try:
            args.forecast = (int(args.forecast[0]), args.forecast[1])
        except ValueError:
            parser.error(f"--forecast: the horizon must be an integer, got {args.forecast[0]!r}")
        if args.forecast[0] < 0:
            parser.error("--forecast: the horizon must not be negative")
    return args


def apply_overrides(hp: HyperParams, args) -> HyperParams:
    """main.py:112-128 (theta values are parsed as floats here; the reference keeps strings, a bug)."""
    if args.T is not None:
        hp.T = int(args.T)
    if args.impute is not None:
        hp.impute = int(args.impute)
    if args.theta is not None:
        vals = []
        for t in args.theta:
            vals += [float(v) for v in str(t).split(",") if v.strip()]
        hp.theta = vals
    if args.x0 is not None:
        hp.x0 = float(args.x0)
    if args.obs_std is not None:
        hp.obs_std = float(args.obs_std)
    if args.kernel_len is not None:
        hp.kernel_len = int(args.kernel_len)
    if args.batch_dims is not None:
        hp.batch_dims = int(args.batch_dims)
    if args.feat_window is not None:
        hp.feat_window = int(args.feat_window)
    if getattr(args, "p", None) is not None:
        hp.p = int(args.p)
    return hp
