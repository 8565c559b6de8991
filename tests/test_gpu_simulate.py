"""vissm_sde_simulate (ops.sde_simulate) on the GPU against replays of the same chain in numpy (tests/sim_util.py).

The kernel draws its normals itself; ops.normal_base(seed, row0, B, NS * H, 0) returns exactly the numbers it
consumes (NS = S state normals per step, then S observation normals when observations are asked for), so the chain
is replayed from them in float64, nothing rounded.  The bar comes from the references alone: the same replay in
numpy float32 arithmetic deviates from the float64 one by at most e32 (measured in the test, per case), and the
kernel must stay within 8 * max(e32, 2^-20 * scale) of the float64 replay, scale = the column's mean absolute value;
the factor 8 covers fused multiply-adds and the hardware exp / sqrt, which the numpy fp32 replay does not have.
Chunked, sharded and repeated calls are compared bitwise."""
import numpy as np
import pytest
import torch

from tests import sim_util as SU

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 0x51D5EED
OBS_STD = {SU.AR: 1.0, SU.LV: 1.0, SU.FHN: 0.1}


def _tile():
    from viforssms_amd import _lib
    return _lib.SIM_TILE


def _inputs(model, B, rng):
    """Dynamics in their stable range: AR theta_1 in [0.5, 0.95]; LV rates and FHN raw parameters within 10 % of the
    generators' true values; SV theta = (0, -0.5, log 0.5, log 0.2) at x = (1, -1)."""
    P, S = SU.P_OF[model], SU.S_OF[model]
    true = np.asarray(SU.TRUE_THETA[model])
    if model == SU.AR:
        th = true * rng.uniform(0.9, 1.1, (B, P))
        th[:, 1] = rng.uniform(0.5, 0.95, B)
    elif model == SU.LV:
        th = true + np.log(rng.uniform(0.9, 1.1, (B, P)))
    elif model == SU.FHN:
        th = true * rng.uniform(0.9, 1.1, (B, P))
    else:
        th = np.tile(true, (B, 1))
    x0 = np.asarray(SU.TRUE_X[model]) * (rng.uniform(0.9, 1.1, (B, S)) if model != SU.SV else np.ones((B, S)))
    return th.astype(np.float32), x0.astype(np.float32)


def _simulate(model, th, x0, H, row0=0, t0=0, obs=False, seed=SEED):
    from viforssms_amd import ops
    x, y, xe = ops.sde_simulate(model, torch.as_tensor(th, device=DEV), torch.as_tensor(x0, device=DEV), H,
                                SU.DT[model], seed, row0, t0=t0, obs_std=OBS_STD[model] if obs else None)
    torch.cuda.synchronize()
    return x.cpu().numpy(), (y.cpu().numpy() if y is not None else None), xe.cpu().numpy()


def _normals(model, B, H, row0=0, obs=False, seed=SEED):
    from viforssms_amd import ops
    NS = SU.S_OF[model] * (2 if obs else 1)
    eps, _ = ops.normal_base(seed, row0, B, NS * H, 0, DEV)
    return eps.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _bar(ref64, ref32):
    """8 * max(e32, 2^-20 * column mean |ref64|) per column [S, H] and e32, over the entries finite in both replays."""
    both = np.isfinite(ref64) & np.isfinite(ref32)
    e32 = float(np.max(np.abs(ref32.astype(np.float64) - ref64)[both])) if both.any() else 0.0
    with np.errstate(invalid="ignore"):
        scale = np.nan_to_num(np.nanmean(np.abs(ref64), axis=0), nan=0.0)
    return 8.0 * np.maximum(e32, 2.0 ** -20 * scale), e32


def _shapes():
    T = _tile()
    Bs, Hs = [1, 63, 64, 65, 130], [1, 3, 4, 5, T - 1, T, T + 1, 2 * T + 3]
    return sorted({(B, T + 1) for B in Bs} | {(65, H) for H in Hs})


@pytest.mark.parametrize("B,H", _shapes())
@pytest.mark.parametrize("model,obs", [(SU.AR, False), (SU.AR, True), (SU.LV, False), (SU.LV, True), (SU.SV, False),
                                       (SU.FHN, False)])
def test_kernel_replays_its_normals(model, obs, B, H):
    rng = np.random.default_rng(1000 * model + 10 * B + H)
    th, x0 = _inputs(model, B, rng)
    row0 = 7 + 1000 * B
    nn = _normals(model, B, H, row0, obs)
    os_ = OBS_STD[model] if obs else None
    r64 = SU.replay(model, x0, th, SU.DT[model], nn, H, os_, np.float64)
    r32 = SU.replay(model, x0, th, SU.DT[model], nn, H, os_, np.float32)
    assert np.isfinite(r64[0]).all(), "the stable-range inputs left the domain in the float64 replay"
    x, y, xe = _simulate(model, th, x0, H, row0, obs=obs)
    assert x.shape == (B, SU.S_OF[model], H) and xe.shape == (B, SU.S_OF[model])
    bar, e32 = _bar(r64[0], r32[0])
    dev = np.abs(x - r64[0])
    print(f"model {model} obs {obs} B {B} H {H}: e32 {e32:.3e} kernel deviation {dev.max():.3e} "
          f"(largest share of its bar {np.max(dev / bar):.3f})")
    assert np.all(dev <= bar)
    assert np.array_equal(xe, x[:, :, -1])
    if obs:
        ybar, ye32 = _bar(r64[1], r32[1])
        assert np.all(np.abs(y - r64[1]) <= ybar), (ye32, np.abs(y - r64[1]).max())
    else:
        assert y is None


@pytest.mark.parametrize("model,obs", [(SU.AR, False), (SU.LV, True)])
def test_chunked_horizon_is_bitwise_the_single_call(model, obs):
    """AR consumes one normal per step (four steps per Philox group), LV with observations four (one step per
    group): a restart at t0 continues the stream inside a group and across the tile boundary."""
    T = _tile()
    B, H = 70, 2 * T + 3
    th, x0 = _inputs(model, B, np.random.default_rng(5))
    x, y, xe = _simulate(model, th, x0, H, row0=11, obs=obs)
    for t0 in (1, 3, 5, T, T + 2):
        xa, ya, xea = _simulate(model, th, x0, t0, row0=11, obs=obs)
        xb, yb, xeb = _simulate(model, th, xea, H - t0, row0=11, t0=t0, obs=obs)
        assert np.array_equal(_bits(np.concatenate([xa, xb], 2)), _bits(x)), t0
        assert np.array_equal(_bits(xeb), _bits(xe)), t0
        if obs:
            assert np.array_equal(_bits(np.concatenate([ya, yb], 2)), _bits(y)), t0
    # three chunks, the middle one inside a tile
    xa, _, ea = _simulate(model, th, x0, 2, row0=11, obs=obs)
    xb, _, eb = _simulate(model, th, ea, 7, row0=11, t0=2, obs=obs)
    xc, _, ec = _simulate(model, th, eb, H - 9, row0=11, t0=9, obs=obs)
    assert np.array_equal(_bits(np.concatenate([xa, xb, xc], 2)), _bits(x)) and np.array_equal(_bits(ec), _bits(xe))


@pytest.mark.parametrize("model,obs", [(SU.AR, False), (SU.LV, True), (SU.FHN, False)])
def test_stream_is_keyed_by_the_global_row(model, obs):
    T = _tile()
    B, H = 130, T + 1
    th, x0 = _inputs(model, B, np.random.default_rng(6))
    x, y, xe = _simulate(model, th, x0, H, row0=40, obs=obs)
    x2, y2, xe2 = _simulate(model, th, x0, H, row0=40, obs=obs)
    assert np.array_equal(_bits(x), _bits(x2)) and np.array_equal(_bits(xe), _bits(xe2))     # run to run
    xa, ya, xea = _simulate(model, th[:65], x0[:65], H, row0=40, obs=obs)
    xb, yb, xeb = _simulate(model, th[65:], x0[65:], H, row0=40 + 65, obs=obs)
    assert np.array_equal(_bits(np.concatenate([xa, xb])), _bits(x))
    assert np.array_equal(_bits(np.concatenate([xea, xeb])), _bits(xe))
    if obs:
        assert np.array_equal(_bits(y), _bits(y2)) and np.array_equal(_bits(np.concatenate([ya, yb])), _bits(y))
    other, _, _ = _simulate(model, th, x0, H, row0=41, obs=obs)
    assert not np.array_equal(other, x)


def test_dead_rows():
    """LV started next to the boundary, x = (0.1 .. 1.5, 100) at the generator's theta: some rows leave the positive
    orthant within 40 steps and some do not (with numpy's own normals about 37 % do; from 0.3 .. 3 about 15 %, too
    close to the 10 % this test wants on either side to hold for whatever seed).  Every row's first NaN step is the
    float64 replay's exit step; before it the bar of test_kernel_replays_its_normals holds; from it on x, y and
    x_end are NaN.  A row is left out of
    the exit-step comparison only if its float64 replay comes within 1e-3 |step increment| of the boundary at a step
    up to its exit, where a rounding difference may legitimately flip the decision."""
    B, H = 256, 40
    rng = np.random.default_rng(12)
    th = np.tile(np.asarray(SU.TRUE_THETA[SU.LV], np.float32), (B, 1))
    x0 = np.stack([rng.uniform(0.1, 1.5, B), np.full(B, 100.0)], 1).astype(np.float32)
    nn = _normals(SU.LV, B, H, row0=3, obs=True)
    x64, y64, _, prev, raw, exit64 = SU.replay(SU.LV, x0, th, 0.1, nn, H, OBS_STD[SU.LV], np.float64)
    x32, y32, *_ = SU.replay(SU.LV, x0, th, 0.1, nn, H, OBS_STD[SU.LV], np.float32)
    died = exit64 < H
    assert died.mean() >= 0.10 and (~died).mean() >= 0.10, died.mean()
    with np.errstate(invalid="ignore"):
        upto = np.arange(H)[None, None, :] <= exit64[:, None, None]
        near = (np.abs(raw) <= 1e-3 * np.abs(raw - prev)) & upto
    left_out = near.any((1, 2))
    assert left_out.mean() <= 0.05, left_out.mean()

    x, y, xe = _simulate(SU.LV, th, x0, H, row0=3, obs=True)
    first_nan = np.where(np.isnan(x).any(1).any(1), np.isnan(x).any(1).argmax(1), H)
    keep = ~left_out
    print(f"dead rows: {died.sum()} of {B} die in the float64 replay, {left_out.sum()} left out")
    assert np.array_equal(first_nan[keep], exit64[keep])
    t = np.arange(H)[None, None, :]
    after = np.broadcast_to(t >= first_nan[:, None, None], x.shape)
    assert np.isnan(x[after]).all() and np.isnan(y[after]).all()
    assert not np.isnan(x[~after]).any() and not np.isnan(y[~after]).any()
    assert np.array_equal(np.isnan(xe).all(1), first_nan < H) and np.array_equal(np.isnan(xe).any(1), first_nan < H)
    before = ~after & keep[:, None, None]
    for got, r64, r32 in ((x, x64, x32), (y, y64, y32)):
        bar, e32 = _bar(r64, r32)
        dev = np.where(before, np.abs(got - r64), 0.0)
        print(f"dead rows: e32 {e32:.3e} kernel deviation before the exit {np.nanmax(dev):.3e}")
        assert np.all(dev <= bar[None])
    alive_rows = first_nan == H
    assert np.array_equal(xe[alive_rows], x[alive_rows][:, :, -1])

    # a dead start is NaN throughout, a dead row handed on through x_end stays dead
    bad0 = np.asarray([[-1.0, 100.0], [np.nan, 100.0], [100.0, np.inf], [100.0, 100.0]], np.float32)
    xb, yb, xeb = _simulate(SU.LV, th[:4], bad0, 9, obs=True)
    assert np.isnan(xb[:3]).all() and np.isnan(yb[:3]).all() and np.isnan(xeb[:3]).all()
    assert np.isfinite(xb[3]).all() and np.isfinite(yb[3]).all()
    xc, _, xec = _simulate(SU.LV, th[:4], xeb, 5, t0=9, obs=True)
    assert np.isnan(xc[:3]).all() and np.isnan(xec[:3]).all() and np.isfinite(xc[3]).all()


def test_empty_horizon_and_refusals():
    from viforssms_amd import _lib, ops
    th, x0 = _inputs(SU.LV, 5, np.random.default_rng(1))
    tht, x0t = torch.as_tensor(th, device=DEV), torch.as_tensor(x0, device=DEV)
    x, y, xe = ops.sde_simulate(SU.LV, tht, x0t, 0, 0.1, 1, 0, obs_std=1.0)
    assert tuple(x.shape) == (5, 2, 0) and tuple(y.shape) == (5, 2, 0) and torch.equal(xe, x0t)
    x, y, xe = ops.sde_simulate(SU.AR, tht, x0t[:, :1].contiguous(), 0, 1.0, 1, 0)
    assert tuple(x.shape) == (5, 1, 0) and y is None
    with pytest.raises(_lib.VissmError, match="GPU only"):
        ops.sde_simulate(SU.LV, tht.cpu(), x0t.cpu(), 4, 0.1, 1, 0)
    with pytest.raises(_lib.VissmError, match="SV"):
        ops.sde_simulate(SU.SV, torch.zeros(5, 4, device=DEV), x0t, 4, 0.1, 1, 0, obs_std=1.0)
    with pytest.raises(_lib.VissmError, match="expected"):
        ops.sde_simulate(SU.LV, tht, x0t[:, :1].contiguous(), 4, 0.1, 1, 0)
    with pytest.raises(_lib.VissmError, match="horizon"):
        ops.sde_simulate(SU.LV, tht, x0t, -1, 0.1, 1, 0)
    with pytest.raises(_lib.VissmError, match="horizon"):
        ops.sde_simulate(SU.LV, tht, x0t, 4, 0.1, 1, 0, t0=2 ** 30)
