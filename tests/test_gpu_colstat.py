"""The column-statistics kernels alone (viforssms_amd/csrc/colstat.hip through ops.col_moments / ops.col_order_stats
and summary.column_summary) against numpy on the CPU.

Order statistics are exact: np.sort(x, axis=0)[r], compared with np.array_equal(equal_nan=True), no tolerance.
Moments: |sum - ref| <= 2 B 2^-53 sum|x| (and the same for the squares), the recursive-summation bound for double
accumulation of exactly represented fp32 inputs, times 2; ref = numpy float64 nansum; n_valid exact; two launches
bitwise equal.  Quantiles: np.nanquantile of the float64 copy at rtol 1e-12 (both sides interpolate in float64)."""
import warnings

import numpy as np
import pytest
import torch

from tests.colstat_util import data_classes

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BS = [1, 2, 50, 63, 64, 65, 257, 1031]
NCOLS = [1, 3, 31, 32, 33, 70]
CLASSES = ["normal", "ties", "equal", "last_byte", "mixed"]


def _ranks(B):
    """{0, 1, B//2, B-2, B-1} clipped to the column, with one rank repeated."""
    return np.clip(np.array([0, 1, B // 2, B - 2, B - 1, B // 2]), 0, B - 1)


def _gpu(x, layout="dense"):
    """x on the GPU as a [B, n_cols] view: dense, with a row pitch of n_cols + 5, or starting one float into its
    storage (x[:, 1:]); what lies outside the view is NaN / huge so a read beyond it shows."""
    B, n = x.shape
    if layout == "dense":
        return torch.from_numpy(x).to(DEV)
    pad = 5 if layout == "pitch" else 1
    base = torch.full((B, n + pad), float("nan") if layout == "pitch" else 3e38, device=DEV)
    view = base[:, :n] if layout == "pitch" else base[:, 1:]
    view.copy_(torch.from_numpy(x))
    assert not view.is_contiguous() or B == 1
    return view


def _check_order_stats(x, ranks, layout="dense"):
    from viforssms_amd import ops
    got = ops.col_order_stats(_gpu(x, layout), torch.from_numpy(np.asarray(ranks)).to(torch.int32)).cpu().numpy()
    srt = np.sort(x, axis=0)
    r = np.asarray(ranks)
    want = srt[r] if r.ndim == 1 else np.take_along_axis(srt, r.T, axis=0)      # [n_ranks, n_cols]
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.array_equal(got, want, equal_nan=True), np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5]


def _check_moments(x, layout="dense"):
    from viforssms_amd import ops
    xg = _gpu(x, layout)
    sums, n_valid = ops.col_moments(xg)
    sums2, n_valid2 = ops.col_moments(xg)
    assert torch.equal(sums.view(torch.int64), sums2.view(torch.int64)) and torch.equal(n_valid, n_valid2)
    sums, n_valid = sums.cpu().numpy(), n_valid.cpu().numpy()
    x64 = x.astype(np.float64)
    B = x.shape[0]
    assert np.array_equal(n_valid, (~np.isnan(x)).sum(0))
    for got, v in ((sums[0], x64), (sums[1], x64 * x64)):
        ref, mag = np.nansum(v, axis=0), np.nansum(np.abs(v), axis=0)
        err, bound = np.abs(got - ref), 2.0 * B * 2.0 ** -53 * mag
        print("moments max err / bound", float(np.max(err / np.maximum(bound, 1e-300))))
        assert np.all(err <= bound), (err.max(), bound[np.argmax(err)])


def _finite(x):
    """The moments' inputs: +-inf (whose sum is NaN on both sides) replaced by +-1e30, the NaNs kept."""
    return np.where(np.isinf(x), np.sign(x) * np.float32(1e30), x).astype(np.float32)


@pytest.mark.parametrize("n_cols", NCOLS)
@pytest.mark.parametrize("B", BS)
def test_order_statistics_and_moments(B, n_cols):
    rng = np.random.default_rng(1000 * B + n_cols)
    for name, x in data_classes(B, rng, n_cols).items():
        _check_order_stats(x, _ranks(B))
        _check_moments(_finite(x))


@pytest.mark.parametrize("layout", ["pitch", "offset"])
def test_pitched_and_offset_views(layout):
    rng = np.random.default_rng(7)
    B, n = 257, 33
    for name, x in data_classes(B, rng, n).items():
        _check_order_stats(x, _ranks(B), layout)
        _check_moments(_finite(x), layout)


def test_several_row_slabs_and_column_tiles():
    rng = np.random.default_rng(8)
    B, n = 4099, 130
    for name, x in data_classes(B, rng, n).items():
        _check_order_stats(x, _ranks(B))
        _check_moments(_finite(x))


def test_sixteen_ranks_and_per_column_ranks():
    rng = np.random.default_rng(9)
    B, n = 1031, 70
    data = data_classes(B, rng, n)
    sixteen = np.clip(np.array([0, 1, 2, 7, 100, 101, B // 4, B // 2 - 1, B // 2, B // 2, B // 2 + 1, 3 * B // 4, B - 20,
                                B - 3, B - 2, B - 1]), 0, B - 1)
    for name in CLASSES:
        _check_order_stats(data[name], sixteen)
        _check_order_stats(data[name], rng.integers(0, B, (n, 16)))      # every column its own 16 ranks
        _check_order_stats(data[name], rng.integers(0, B, (n, 5)), "offset")
    # int64 ranks on the host, a single rank
    _check_order_stats(data["normal"], np.array([B // 2], dtype=np.int64))


def test_rank_and_shape_checks():
    from viforssms_amd import _lib, ops
    x = torch.zeros(8, 3, device=DEV)
    for bad in ([8], [-1], [0, 9]):
        with pytest.raises(_lib.VissmError, match="ranks outside"):
            ops.col_order_stats(x, torch.tensor(bad, dtype=torch.int32))
    with pytest.raises(_lib.VissmError, match="ranks per column"):
        ops.col_order_stats(x, torch.zeros(17, dtype=torch.int32))
    with pytest.raises(_lib.VissmError, match="unit inner stride"):
        ops.col_moments(torch.zeros(3, 8, device=DEV).t())
    with pytest.raises(_lib.VissmError):
        ops.col_moments(x.double())
    # ranks that live on the device are not read back: the narrowing step clamps them into the column
    got = ops.col_order_stats(torch.arange(24, dtype=torch.float32, device=DEV).view(8, 3),
                              torch.tensor([-5, 100], dtype=torch.int32, device=DEV)).cpu().numpy()
    assert np.array_equal(got, np.array([[0, 1, 2], [21, 22, 23]], dtype=np.float32))


PROBS = (0.0, 0.025, 0.25, 0.5, 0.75, 0.975, 1.0)


@pytest.mark.parametrize("B,n_cols", [(1, 3), (2, 3), (63, 31), (1031, 70), (4099, 130)])
def test_column_summary_matches_numpy(B, n_cols):
    from viforssms_amd.summary import column_summary
    rng = np.random.default_rng(B)
    data = data_classes(B, rng, n_cols)
    for name in ("normal", "ties", "equal", "last_byte"):
        x = data[name]
        s = column_summary(_gpu(x, "offset"), PROBS)
        x64 = x.astype(np.float64)
        want = np.nanquantile(x64, PROBS, axis=0)
        assert s["quantiles"].shape == (len(PROBS), n_cols) and s["quantiles"].dtype == np.float64
        assert np.allclose(s["quantiles"], want, rtol=1e-12, atol=0.0), name
        assert np.array_equal(s["n_valid"], np.full(n_cols, B))
        # mean: the moments' bound over n; sd from E x^2 - mean^2 in float64: its cancellation leaves an absolute
        # error of a few 2^-53 E x^2 in the variance
        assert np.all(np.abs(s["mean"] - x64.mean(0)) <= 2.0 * B * 2.0 ** -53 * np.abs(x64).mean(0))
        var_err = 8.0 * (B + 2) * 2.0 ** -53 * (x64 * x64).mean(0)
        assert np.all(np.abs(s["sd"] ** 2 - x64.var(0)) <= var_err), name


def test_column_summary_nan_semantics():
    """np.nanmean / np.nanstd / np.nanquantile: NaNs left out column by column, an all-NaN column gives NaN."""
    from viforssms_amd.summary import DEFAULT_PROBS, column_summary
    rng = np.random.default_rng(11)
    B, n = 257, 33
    x = (10 + 3 * rng.standard_normal((B, n))).astype(np.float32)
    x[rng.random((B, n)) < 0.2] = np.nan
    x[:, 4] = np.nan
    x[1:, 5] = np.nan
    x[0, 5] = 7.25
    s = column_summary(_gpu(x), DEFAULT_PROBS)
    x64 = x.astype(np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)     # numpy warns about the all-NaN column
        want_q, want_m, want_v = np.nanquantile(x64, DEFAULT_PROBS, axis=0), np.nanmean(x64, 0), np.nanvar(x64, 0)
        mean_abs, mean_sq = np.nanmean(np.abs(x64), 0), np.nanmean(x64 * x64, 0)
    assert np.array_equal(s["n_valid"], (~np.isnan(x)).sum(0))
    assert np.allclose(s["quantiles"], want_q, rtol=1e-12, atol=0.0, equal_nan=True)
    assert np.isnan(s["quantiles"][:, 4]).all() and np.isnan(s["mean"][4]) and np.isnan(s["sd"][4])
    ok = s["n_valid"] > 0
    # the bounds of test_column_summary_matches_numpy
    assert np.all(np.abs(s["mean"] - want_m)[ok] <= (2.0 * B * 2.0 ** -53 * mean_abs)[ok])
    assert np.all(np.abs(s["sd"] ** 2 - want_v)[ok] <= (8.0 * (B + 2) * 2.0 ** -53 * mean_sq)[ok])
    assert s["sd"][5] == 0.0 and s["mean"][5] == float(x[0, 5]) and np.all(s["quantiles"][:, 5] == float(x[0, 5]))
