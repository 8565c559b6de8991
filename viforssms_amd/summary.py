"""Posterior summaries computed where the samples are: per-column mean, sd and quantiles of a sample-major
[B, n_cols] GPU matrix (the latent path's credible bands over time, the marginals of theta), exact over all
data-parallel ranks' samples without gathering them.

The reference gets there through the host: VI_SSM.save_paths writes every sample with np.savetxt (AR.py:323-362) and
vis.py takes the quantiles of that file offline.  Here the moments come from vissm_col_moments and the quantiles from
the order statistics of a 4-pass radix select (vissm_col_select_*; ops.col_order_stats), whose only cross-rank
quantity is an integer histogram.  A few KB reach the host."""
from __future__ import annotations

from typing import Dict, Sequence

import numpy as np
import torch

from . import _lib, ops

DEFAULT_PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)
MAX_PROBS = _lib.COLSTAT_MAX_RANKS // 2   # two order statistics per quantile


def _check_probs(probs: Sequence[float]) -> np.ndarray:
    p = np.asarray(list(probs), dtype=np.float64)
    if p.ndim != 1 or not 1 <= p.size <= MAX_PROBS:
        raise ValueError(f"1..{MAX_PROBS} quantile probabilities expected, got {p.size}")
    if not np.all((p >= 0.0) & (p <= 1.0)):
        raise ValueError("quantile probabilities must lie in [0, 1]")
    return p


def column_summary(x: torch.Tensor, probs: Sequence[float] = DEFAULT_PROBS, dist=None) -> Dict[str, np.ndarray]:
    """mean [n_cols], sd [n_cols] (population, ddof = 0), quantiles [len(probs), n_cols] (numpy's default 'linear'
    method) and n_valid [n_cols] of the columns of x [B, n_cols] (fp32 GPU tensor, unit inner stride, any row stride
    and storage offset), as float64 / int64 host arrays with the semantics of np.nanmean, np.nanstd and
    np.nanquantile: NaN entries are left out, a column of NaNs gives NaN.  dist (vi_ssm.DistCtx): the summary of
    the union of every rank's rows, the same on every rank.

    Per column pos = (n_valid - 1) p; the order statistics of ranks floor(pos) and ceil(pos) are selected on the
    device (the ranks are built there from n_valid) and interpolated in float64 on the host.  One host
    synchronisation, the final copy."""
    p = _check_probs(probs)
    sums, n_valid = ops.col_moments(x)
    if dist is not None and dist.world > 1:
        dist.all_reduce_(sums)
        dist.all_reduce_(n_valid)
    pd = torch.as_tensor(p, device=x.device)                                       # [Q] float64
    pos = (n_valid.to(torch.float64) - 1.0).clamp_min(0.0).unsqueeze(1) * pd      # [n_cols, Q]
    ranks = torch.cat([pos.floor(), pos.ceil()], 1).to(torch.int32)               # [n_cols, 2 Q]
    stats = ops.col_order_stats(x, ranks, dist)                                    # [2 Q, n_cols]
    sums_h, n_h, stats_h = sums.cpu().numpy(), n_valid.cpu().numpy().astype(np.int64), stats.cpu().numpy()

    Q = p.size
    n = n_h.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(n_h > 0, sums_h[0] / n, np.nan)
        var = np.where(n_h > 0, sums_h[1] / n - mean * mean, np.nan)
    sd = np.sqrt(np.maximum(var, 0.0))
    pos_h = np.maximum(n - 1.0, 0.0)[None, :] * p[:, None]                         # the device's products, [Q, n_cols]
    t = pos_h - np.floor(pos_h)
    lo, hi = stats_h[:Q].astype(np.float64), stats_h[Q:].astype(np.float64)
    with np.errstate(invalid="ignore"):
        diff = hi - lo
        # numpy's _lerp: a + (b - a) t, from b's side for t >= 0.5, and exactly a where the two coincide
        q = np.where(t >= 0.5, hi - diff * (1.0 - t), lo + diff * t)
        q = np.where(hi == lo, lo, q)
    q = np.where(n_h[None, :] > 0, q, np.nan)
    return {"mean": mean, "sd": sd, "quantiles": q, "n_valid": n_h}
