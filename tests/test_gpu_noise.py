"""The base noise on the GPU (vissm_normal_base, vissm_normal_base_dev, vissm_base_logprob, the forecast kernel's own
copy of the draw, Engine.draw) against tests/philox_ref.py, the numpy reference written from the Philox paper and
the contract in include/vissm.h.

Two bars, kept apart:

  identity  |gpu - ref| <= 1e-3 everywhere.  A wrong bit in the counter, the key or a round moves almost every entry
            by O(1); a right stream cannot be 1e-3 off unless a transcendental is broken.
  accuracy  |gpu - ref| <= ACC_FACTOR * e32.  e32 is the reference's own fp32 error: the largest deviation of the
            numpy float32 restatement of Box-Muller (philox_ref.normals(dtype=float32)) from the float64 one, both
            from the same exact uniforms, over the 512 x 1024 draws of seed 1, rows 0 .. 511 (about 1.5e-6: the
            rounding of the angle 2 pi u at a radius of up to 5.5).  It is measured once per session on that fixed
            sample rather than on each case's own draws: the small cases (one row of one column) hold too few
            draws to meet the large radii that set the error's scale, and a bar from them would be luck.  The
            distribution test measures it again on its own 2048 x 2048 draws.  The factor 8 is the margin
            tests/test_gpu_simulate.py grants fused multiply-adds and hardware transcendentals.

Everything else is bitwise or a count: canaries around the buffers, the device-offset entry point, the engine's row
bookkeeping."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from tests import philox_ref as PR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
IDENTITY_TOL = 1e-3
ACC_FACTOR = 8.0
THETA_XOR = 0x5DEECE66D

B_LIST = [1, 3, 5, 130]
L_SHORT = [1, 2, 3, 4, 5, 63, 64]                       # one thread per row (L <= 64)
L_LONG = [65, 66, 67, 127, 255, 256, 257, 1001]         # one wave per row: tails of 1 .. 3 columns, odd rows
SEEDS = [1, 2 ** 32, 0xFFFFFFFF00000001, 2 ** 64 - 1]
OFFSETS = [0, 2 ** 32 - 3, 2 ** 40 + 7, 2 ** 63 + 1]
DIST_KEYS = [1, 1 ^ THETA_XOR, 12345678901234567]
SENTINEL = 0x7FA5C3E1                                   # a NaN bit pattern no draw produces


def _lib_and_stream():
    from viforssms_amd import _lib
    return _lib, _lib.load(), _lib.stream_handle(torch.device(DEV))


@functools.lru_cache(maxsize=1)
def _e32():
    r64 = PR.normals(1, 0, 512, 1024)
    r32 = PR.normals(1, 0, 512, 1024, dtype=np.float32)
    return float(np.max(np.abs(r32.astype(np.float64) - r64)))


def _bar():
    return ACC_FACTOR * _e32()


@functools.lru_cache(maxsize=32)
def _ref(seed, offset):
    """Reference rows offset .. offset + 129, 1004 columns: every shape of the stream tests is a corner of it."""
    a = PR.normals(seed, offset, max(B_LIST), 1004)
    a.setflags(write=False)
    return a


def _gpu(seed, offset, B, L, n_last=0):
    from viforssms_amd.ops import normal_base
    eps, lp = normal_base(seed, offset, B, L, n_last, DEV)
    torch.cuda.synchronize()
    return eps.cpu().numpy(), lp.cpu().numpy()


def _lane_dev(dev):
    """largest deviation on the cos lanes (even columns) and on the sin lanes (odd columns)"""
    return float(dev[:, 0::2].max(initial=0.0)), float(dev[:, 1::2].max(initial=0.0))


# ---- a. stream identity and Box-Muller accuracy ---------------------------------------------------------------
@pytest.mark.parametrize("L", L_SHORT + L_LONG)
def test_stream_is_the_reference_stream(L):
    bar, worst = _bar(), [0.0, 0.0]
    for seed in SEEDS:
        for offset in OFFSETS:
            ref = _ref(seed, offset)
            for B in B_LIST:
                eps, _ = _gpu(seed, offset, B, L)
                assert eps.shape == (B, L) and eps.dtype == np.float32
                dev = np.abs(eps.astype(np.float64) - ref[:B, :L])
                where = f"seed {seed:#x} offset {offset:#x} B {B} L {L}"
                assert np.all(dev <= IDENTITY_TOL), f"not the reference stream: {where}, {int((dev > IDENTITY_TOL).sum())} entries"
                c, s = _lane_dev(dev)
                worst = [max(worst[0], c), max(worst[1], s)]
                assert np.all(dev <= bar), f"Box-Muller accuracy: {where}, {dev.max():.3e} > {bar:.3e}"
    print(f"L {L}: e32 {_e32():.3e}, largest deviation cos lanes {worst[0]:.3e} sin lanes {worst[1]:.3e} "
          f"(bar {bar:.3e} = {ACC_FACTOR:g} e32)")


# ---- b. the ends of (0, 1] ------------------------------------------------------------------------------------
# (row, group, word index 0..3 = x y z w) at L = 1024, seed 1, found by searching the reference
R_MAX = math.sqrt(48.0 * math.log(2.0))                 # sqrt(-2 ln 2^-24)
ENDS = {
    "u1_min": [(37979, 190, 0), (31399, 40, 2)],
    "u1_one": [(25942, 132, 0)],
    "u2_one": [(4092, 253, 1), (33084, 198, 3)],
    "u2_min": [(50140, 137, 1), (55962, 105, 3)],
}


def _end_case(row, g, word, want_top24):
    w = PR.words(1, row, 1, 1024)[0, g]
    assert int(w[word]) >> 8 == want_top24, (row, g, word, hex(int(w[word])))
    eps, _ = _gpu(1, row, 1, 1024)
    ref = PR.normals(1, row, 1, 1024)
    c0 = 4 * g + 2 * (word // 2)                        # the pair's cos column: x, y -> 4g; z, w -> 4g + 2
    dev = np.abs(eps.astype(np.float64) - ref)
    assert np.all(dev <= _bar()), (row, dev.max())
    return eps[0].astype(np.float64), ref[0], c0


@pytest.mark.parametrize("row,g,word", ENDS["u1_min"])
def test_smallest_u1_gives_the_largest_radius(row, g, word):
    eps, ref, c0 = _end_case(row, g, word, 0)
    assert abs(np.hypot(ref[c0], ref[c0 + 1]) - R_MAX) < 1e-12
    print(f"row {row}: pair {eps[c0]:.7f} {eps[c0 + 1]:.7f}, radius {np.hypot(eps[c0], eps[c0 + 1]):.7f} vs {R_MAX:.7f}")
    assert abs(np.hypot(eps[c0], eps[c0 + 1]) - R_MAX) <= _bar()


@pytest.mark.parametrize("row,g,word", ENDS["u1_one"])
def test_u1_of_one_gives_a_zero_radius(row, g, word):
    eps, ref, c0 = _end_case(row, g, word, 0xFFFFFF)
    assert ref[c0] == 0.0 and ref[c0 + 1] == 0.0
    assert eps[c0] == 0.0 and eps[c0 + 1] == 0.0, (eps[c0], eps[c0 + 1])       # +-0.0, not NaN from sqrt(-0)


@pytest.mark.parametrize("row,g,word", ENDS["u2_one"])
def test_u2_of_one_is_a_whole_revolution(row, g, word):
    eps, ref, c0 = _end_case(row, g, word, 0xFFFFFF)
    u = PR.uniforms(PR.words(1, row, 1, 1024)[0, g])
    radius = math.sqrt(-2.0 * math.log(u[word - 1]))
    assert abs(eps[c0] - radius) <= _bar() and abs(eps[c0 + 1]) <= _bar(), (eps[c0], eps[c0 + 1], radius)


@pytest.mark.parametrize("row,g,word", ENDS["u2_min"])
def test_smallest_u2(row, g, word):
    _end_case(row, g, word, 0)


# ---- c. nothing outside the buffers ---------------------------------------------------------------------------
PAD = 64


@pytest.mark.parametrize("L", L_SHORT + L_LONG)
def test_nothing_is_written_outside_the_buffers(L):
    _lib, lib, st = _lib_and_stream()
    for B in (1, 3, 5):
        big = torch.full((PAD + B * L + PAD,), SENTINEL, dtype=torch.int32, device=DEV)
        lpb = torch.full((PAD + B + PAD,), SENTINEL, dtype=torch.int32, device=DEV)
        _lib.check(lib.vissm_normal_base(ctypes.c_uint64(1), ctypes.c_uint64(9), big.data_ptr() + 4 * PAD,
                                         lpb.data_ptr() + 4 * PAD, B, L, L, st), "vissm_normal_base")
        torch.cuda.synchronize()
        e, p = big.cpu().numpy(), lpb.cpu().numpy()
        assert np.all(e[:PAD] == SENTINEL) and np.all(e[PAD + B * L:] == SENTINEL), (B, L)
        assert np.all(p[:PAD] == SENTINEL) and np.all(p[PAD + B:] == SENTINEL), (B, L)
        inner = e[PAD:PAD + B * L].view(np.float32).reshape(B, L)
        assert np.all(e[PAD:PAD + B * L] != SENTINEL) and np.all(p[PAD:PAD + B] != SENTINEL)  # every entry written
        assert np.all(np.abs(inner.astype(np.float64) - _ref(1, 9)[:B, :L]) <= _bar())


# ---- d. log-probability windows -------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [5, 64, 67, 1001])
def test_logprob_windows(L):
    from viforssms_amd.ops import base_logprob, normal_base
    B = 5
    for n_last in sorted({0, 1, 2, 5, L - 1, L}):
        eps, lp = normal_base(77, 3, B, L, n_last, DEV)
        lp2 = base_logprob(eps, n_last)
        e = eps.double()
        ref = (-0.5 * e[:, L - n_last:] ** 2).sum(1) - 0.5 * math.log(2 * math.pi) * n_last
        assert torch.allclose(lp.double(), ref, rtol=1e-6, atol=1e-6), (L, n_last)
        assert torch.allclose(lp2.double(), ref, rtol=1e-6, atol=1e-6), (L, n_last)
        if n_last == 0:
            assert torch.all(lp == 0.0) and torch.all(lp2 == 0.0)


# ---- e. the row offset read from device memory ----------------------------------------------------------------
@pytest.mark.parametrize("L", [5, 64, 67, 1001])
def test_device_offset_is_bitwise_the_host_offset(L):
    from viforssms_amd.ops import normal_base, normal_base_dev
    for offset in OFFSETS:
        off_dev = torch.tensor([offset - 2 ** 64 if offset >= 2 ** 63 else offset], dtype=torch.int64, device=DEV)
        for B in (3, 130):
            a, alp = normal_base(0xFFFFFFFF00000001, offset, B, L, min(L, 5), DEV)
            b, blp = normal_base_dev(0xFFFFFFFF00000001, off_dev, B, L, min(L, 5))
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (offset, B)
            assert torch.equal(alp.view(torch.int32), blp.view(torch.int32)), (offset, B)


# ---- f. the simulator's second copy of the draw ---------------------------------------------------------------
def _sim_cases():
    from tests import sim_util as SU
    return [(SU.AR, False, 0), (SU.LV, True, 0), (SU.AR, False, 2 ** 22 + 1), (SU.LV, True, 2 ** 20 + 1)]


@pytest.mark.parametrize("model,obs,t0", _sim_cases())
def test_simulator_draws_the_reference_stream(model, obs, t0):
    """One case of test_gpu_simulate.test_kernel_replays_its_normals under a seed and rows with high words set, then
    with a start step whose first Philox group is >= 2^20 (AR: inside a group).  The normals the replay consumes are
    normal_base's, and those are checked against the reference here, so the chain simulate -> normal_base ->
    reference closes."""
    from tests import sim_util as SU
    from tests import test_gpu_simulate as TS
    from viforssms_amd import ops
    seed, row0 = 0xFFFFFFFF00000001, 2 ** 32 - 3
    B, H = 65, TS._tile() + 1
    NS = SU.S_OF[model] * (2 if obs else 1)
    assert (t0 * NS) // 4 >= 2 ** 20 or t0 == 0
    th, x0 = TS._inputs(model, B, np.random.default_rng(1000 * model + 10 * B + H))
    if t0 == 0:
        nn = TS._normals(model, B, H, row0, obs, seed=seed)
    else:
        eps, _ = ops.normal_base(seed, row0, B, NS * (t0 + H), 0, DEV)
        nn = eps[:, NS * t0:].cpu().numpy()
        del eps
    ref = PR.normals(seed, row0, B, NS * H, col0=NS * t0)
    ndev = np.abs(nn.astype(np.float64) - ref)
    assert np.all(ndev <= IDENTITY_TOL) and np.all(ndev <= _bar()), ndev.max()
    os_ = TS.OBS_STD[model] if obs else None
    r64 = SU.replay(model, x0, th, SU.DT[model], nn, H, os_, np.float64)
    r32 = SU.replay(model, x0, th, SU.DT[model], nn, H, os_, np.float32)
    assert np.isfinite(r64[0]).all(), "the stable-range inputs left the domain in the float64 replay"
    x, y, xe = TS._simulate(model, th, x0, H, row0, t0=t0, obs=obs, seed=seed)
    assert x.shape == (B, SU.S_OF[model], H) and xe.shape == (B, SU.S_OF[model])
    bar, e32 = TS._bar(r64[0], r32[0])
    dev = np.abs(x - r64[0])
    print(f"model {model} obs {obs} t0 {t0}: e32 {e32:.3e} kernel deviation {dev.max():.3e}")
    assert np.all(dev <= bar)
    assert np.array_equal(xe, x[:, :, -1])
    if obs:
        ybar, ye32 = TS._bar(r64[1], r32[1])
        assert np.all(np.abs(y - r64[1]) <= ybar), (ye32, np.abs(y - r64[1]).max())
    else:
        assert y is None


# ---- g. distribution on the device ----------------------------------------------------------------------------
def _device_figures(x):
    """philox_ref.distribution_figures on the GPU in float64"""
    n = x.numel()
    flat, _ = torch.sort(x.reshape(-1))
    cdf = 0.5 * (1.0 + torch.special.erf(flat / math.sqrt(2.0)))
    i = torch.arange(1, n + 1, dtype=torch.float64, device=x.device)
    D = max((i / n - cdf).max().item(), (cdf - (i - 1.0) / n).max().item())
    m = x.mean()
    return {"ks": D * math.sqrt(n), "mean": abs(m.item()), "var": abs(((x - m) ** 2).mean().item() - 1.0),
            "m3": abs((x ** 3).mean().item()), "m4": abs((x ** 4).mean().item() - 3.0),
            "lag_col": abs((x[:, :-1] * x[:, 1:]).mean().item()), "lag_row": abs((x[:-1] * x[1:]).mean().item())}


@pytest.mark.parametrize("key", DIST_KEYS)
def test_device_distribution(key):
    from viforssms_amd.ops import normal_base
    eps, _ = normal_base(key, 0, 2048, 2048, 0, DEV)
    x = eps.double()
    caps, fig = PR.distribution_caps(x.numel()), _device_figures(x)
    print(f"key {key:#x}: " + ", ".join(f"{k} {fig[k]:.3e} (cap {caps[k]:.3e})" for k in fig))
    assert torch.isfinite(eps).all()
    for k, v in fig.items():
        assert v <= caps[k], (k, v, caps[k])
    if key == DIST_KEYS[0]:
        other, _ = normal_base(DIST_KEYS[1], 0, 2048, 2048, 0, DEV)
        cross = abs((x * other.double()).mean().item())
        print(f"cross-key product mean {cross:.3e} (cap {caps['cross']:.3e})")
        assert cross <= caps["cross"]
    # the large-sample form of the stream test, e32 measured on these very draws
    r64 = PR.normals_cached(key, 0, 2048, 2048)
    r32 = PR.normals(key, 0, 2048, 2048, dtype=np.float32)
    e32 = float(np.max(np.abs(r32.astype(np.float64) - r64)))
    dev = np.abs(x.cpu().numpy() - r64)
    c, s = _lane_dev(dev)
    print(f"key {key:#x}: e32 {e32:.3e} on these draws, largest deviation cos lanes {c:.3e} sin lanes {s:.3e} "
          f"(ratio {max(c, s) / e32:.2f}, factor {ACC_FACTOR:g})")
    assert np.all(dev <= IDENTITY_TOL)
    assert np.all(dev <= ACC_FACTOR * e32)


# ---- h. how the engine uses the stream ------------------------------------------------------------------------
def test_engine_draw_rows_and_keys():
    from tests.parity_util import build_model
    B = 6
    model = build_model("ar", B, 30, 5, 2, 20, 3, 4, DEV)
    eng, md = model.engine, model.mdef
    seed, L, P, nl = eng.seed, md.kernel_ext, md.P_theta, md.n_logsig
    loc, scale = md.theta_base
    assert 0 < nl <= L
    bar = _bar()
    blocks = []
    for step in (0, 1):
        for rank in (0, 1):
            eps, lp, x0 = eng.draw(step, B, rank * B, 2 * B)
            torch.cuda.synchronize()
            row0 = step * 2 * B + rank * B
            blocks.append(row0)
            ref = PR.normals(seed, row0, B, L)
            dev = np.abs(eps.double().cpu().numpy() - ref)
            assert eps.shape == (B, L) and np.all(dev <= IDENTITY_TOL) and np.all(dev <= bar), (step, rank, dev.max())
            n = PR.normals(seed ^ THETA_XOR, row0, B, P)
            # one multiply and one add in fp32 on top of the draw's own error
            x0_tol = abs(scale) * bar + 2.0 ** -23 * (abs(loc) + np.abs(scale * n))
            assert x0.shape == (B, P) and np.all(np.abs(x0.double().cpu().numpy() - (loc + scale * n)) <= x0_tol)
            lp_ref = (-0.5 * ref[:, L - nl:] ** 2).sum(1) - 0.5 * math.log(2 * math.pi) * nl
            lp_tol = bar * np.abs(ref[:, L - nl:]).sum(1) + 1e-6 * (1.0 + np.abs(lp_ref))
            assert np.all(np.abs(lp.double().cpu().numpy() - lp_ref) <= lp_tol), (step, rank)
    # the four (step, rank) blocks: pairwise disjoint, together rows 0 .. 4 B - 1
    rows = sorted(r for r0 in blocks for r in range(r0, r0 + B))
    assert rows == list(range(4 * B))
