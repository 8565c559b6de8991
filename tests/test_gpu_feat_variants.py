"""Every tile variant of the fused feature branch (vissm_feat_fwd / vissm_feat_bwd: feat_fwd_kernel<8 | 16 | 32>,
feat_bwd_kernel<8 | 16 | 32>) against the float64 reference of tests/feat_ref.py.

pick_kt takes 16 or 32 positions per block only from 512 blocks up, so the shapes of tests/test_gpu_feat.py all run
the 8-position kernels; here VISSM_FEAT_KT / VISSM_FEAT_KT_BWD (read on every call) force each variant at small
shapes on every boundary of its tiling, and vissm_feat_geometry asserts the variant that launches:

* kT in {8, 16, 32} x stride {1, 2}, Lh in {1, kT - 1, kT, kT + 1, 2 kT + 3} (the last partial block, backward
  blocks that own rows but no position, halo rows shared with the neighbour), k in {s, 5, 20, 64},
  (Cin, H) in {(3, 7), (14, 50), (63, 64)}, one and three windows further apart than Lf Cin;
* the two shapes that cross pick_kt's bar on their own (no override);
* mixed variants (the backward reads act rows another forward tiling wrote);
* the largest LDS launch the shape limits allow.

Bars (tests/test_gpu_feat.py's): relative L2 below 2e-6, every element within 1e-4 of the tensor's largest
magnitude; the conv kernel's sample channel exactly zero; a second run bitwise equal.  Forward C and act are bitwise
equal across the three variants (each element is the same fmaf sequence in (j, i) order, then the bias add; the
dense layers do not depend on kT); weight gradients differ by summation order and are held to the float64 bars."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import feat_ref as R  # noqa: E402
from viforssms_amd import _lib  # noqa: E402
from viforssms_amd._lib import check, ptr  # noqa: E402
from viforssms_amd.ops import _feat_params, feat_conv  # noqa: E402

DEV = "cuda:0"
KTS = (8, 16, 32)
NAMES = ["W0", "b0", "W1", "b1", "W2", "b2", "W3", "b3", "conv_w", "conv_b"]
WORST = {}   # test group -> largest error / bar, printed by each test (profiles/: the recorded figures)


def _cases():
    """30 cases: per kT the five Lh x two strides, the other factors cycling so that each value meets each kT"""
    CH = [(3, 7), (14, 50), (63, 64)]
    out = []
    for kt in KTS:
        for i, (s, Lh) in enumerate((s, Lh) for s in (1, 2) for Lh in (1, kt - 1, kt, kt + 1, 2 * kt + 3)):
            k = [s, 5, 20, 64][(i + i // 5) % 4]
            Cin, H = CH[i % 3]
            n_win = [1, 3][(i + i // 5) % 2]
            out.append((kt, s, Lh, k, Cin, H, n_win))
    return out


CASES = _cases()


def test_case_list_covers_every_value_with_every_variant():
    for kt in KTS:
        mine = [c for c in CASES if c[0] == kt]
        assert {c[1] for c in mine} == {1, 2}
        assert {c[2] for c in mine} == {1, kt - 1, kt, kt + 1, 2 * kt + 3}
        assert {5, 20, 64} <= {c[3] for c in mine} and any(c[3] == c[1] for c in mine)
        assert {(c[4], c[5]) for c in mine} == {(3, 7), (14, 50), (63, 64)}
        assert {c[6] for c in mine} == {1, 3}


_cache = {}


def _make(n_win, Lh, Cin, H, k, s, slack=3):
    """inputs (GPU) and the float64 reference (CPU, computed once per shape and shared)"""
    key = (n_win, Lh, Cin, H, k, s, slack)
    if key not in _cache:
        g = torch.Generator(device=DEV).manual_seed(1000 * Lh + 10 * k + s + Cin)
        r = lambda *sh, sc=1.0: torch.randn(*sh, generator=g, device=DEV) * sc
        Lf = s * (Lh - 1) + k + slack
        big = r(n_win, Lf + 7, Cin)
        h0 = big[:, 3:3 + Lf, :]          # windows (Lf + 7) Cin apart, like the AR / FHN window views
        ws = [r(Cin, H, sc=Cin ** -0.5), r(H, sc=0.1)]
        for _ in range(3):
            ws += [r(H, H, sc=H ** -0.5), r(H, sc=0.1)]
        ws += [r(k, 1 + H, H, sc=(k * H) ** -0.5), r(H, sc=0.1)]
        ws = [w.requires_grad_() for w in ws]
        dC = r(n_win, Lh, H)
        ref = R.feat_conv_grads(h0, ws, s, Lh, dC)
        _cache[key] = (h0, ws, dC, ref)
    return _cache[key]


def _desc(h0, ws, s, Lh):
    n_win, Lf, Cin = h0.shape
    return _lib.FeatDesc(n_win, Lf, Cin, ws[6].shape[1], ws[8].shape[0], s, Lh,
                         h0.stride(0) if n_win > 1 else Lf * Cin)


def _force(monkeypatch, kt_f, kt_b):
    for name, v in (("VISSM_FEAT_KT", kt_f), ("VISSM_FEAT_KT_BWD", kt_b)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def _run(h0, ws, s, Lh, dC, want_f, want_b):
    """feat_conv forward + backward; the launched variants asserted through vissm_feat_geometry"""
    d = _desc(h0, ws, s, Lh)
    gf, gb = _lib.feat_geometry(d, False), _lib.feat_geometry(d, True)
    assert gf["kt"] == want_f and gb["kt"] == want_b, (gf, gb)
    assert max(gf["lds_bytes"], gb["lds_bytes"]) <= 160 * 1024
    C = feat_conv(h0, s, Lh, *ws)
    g = torch.autograd.grad(C, ws, dC)
    torch.cuda.synchronize()
    return C.detach(), g


def _hold(tag, group, C, g, ref):
    Cr, _, gr = ref
    worst = 0.0
    for nm, a, b in zip(["C"] + NAMES, [C] + list(g), [Cr] + gr):
        assert a.shape == b.shape
        assert bool(torch.isfinite(a).all()), (tag, nm)
        if nm == "conv_w":      # the sample channel is the flow kernel's: exactly zero here
            assert torch.count_nonzero(a[:, 0, :]) == 0, tag
            a, b = a[:, 1:, :], b[:, 1:, :]
        e2, em = R.rel_l2(a, b), R.max_rel_scale(a, b)
        worst = max(worst, e2 / 2e-6, em / 1e-4)
        assert e2 < 2e-6, (tag, nm, e2)
        assert em <= 1e-4, (tag, nm, em)
    WORST[group] = max(WORST.get(group, 0.0), worst)
    print(f"[feat-variants] {group} {tag}: error / bar {worst:.3f} (group worst {WORST[group]:.3f})")


@pytest.mark.parametrize("kt,s,Lh,k,Cin,H,n_win", CASES)
def test_variant_matches_float64(monkeypatch, kt, s, Lh, k, Cin, H, n_win):
    h0, ws, dC, ref = _make(n_win, Lh, Cin, H, k, s)
    _force(monkeypatch, kt, kt)
    C, g = _run(h0, ws, s, Lh, dC, kt, kt)
    _hold((kt, s, Lh, k, Cin, H, n_win), f"kT{kt}", C, g, ref)
    C2, g2 = _run(h0, ws, s, Lh, dC, kt, kt)
    assert torch.equal(C, C2) and all(torch.equal(a, b) for a, b in zip(g, g2))


@pytest.mark.parametrize("Lh,want", [(256, 32), (128, 16)])
@pytest.mark.parametrize("s", [1, 2])
def test_natural_threshold_shapes(monkeypatch, Lh, want, s):
    """64 windows of 256 / 128 positions: 512 blocks of 32 / 16, the variants pick_kt takes with no override"""
    _force(monkeypatch, None, None)
    h0, ws, dC, ref = _make(64, Lh, 3, 7, 5, s)
    C, g = _run(h0, ws, s, Lh, dC, want, want)
    _hold((Lh, s), "natural", C, g, ref)


@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("kt_f,kt_b", [(8, 32), (32, 8), (16, 32), (32, 16)])
def test_mixed_variants(monkeypatch, kt_f, kt_b, s):
    """the backward reads the act rows a forward of another tiling stored (each forward block stores its own s kT
    rows, the last one all it computed)"""
    h0, ws, dC, ref = _make(3, 2 * 32 + 3, 14, 50, 20, s)
    _force(monkeypatch, kt_f, kt_b)
    C, g = _run(h0, ws, s, 67, dC, kt_f, kt_b)
    _hold((kt_f, kt_b, s), "mixed", C, g, ref)


def test_lds_extreme(monkeypatch):
    """kT = 32, s = 2, k = 64, H = 64, Cin = 63: 83,460 B forward, 124,800 B backward of dynamic LDS"""
    h0, ws, dC, ref = _make(3, 67, 63, 64, 64, 2)
    _force(monkeypatch, 32, 32)
    d = _desc(h0, ws, 2, 67)
    assert _lib.feat_geometry(d, False)["lds_bytes"] == 83460
    assert _lib.feat_geometry(d, True)["lds_bytes"] == 124800
    C, g = _run(h0, ws, 2, 67, dC, 32, 32)
    _hold("k64 H64 Cin63 s2", "lds_extreme", C, g, ref)


def _fwd_direct(h0, ws, s, Lh):
    """vissm_feat_fwd at the C ABI into NaN-filled C and act"""
    n_win, Lf, _ = h0.shape
    H = ws[6].shape[1]
    d = _desc(h0, ws, s, Lh)
    C = torch.full((n_win, Lh, H), float("nan"), device=DEV)
    act = torch.full((4, n_win, Lf, H), float("nan"), device=DEV)
    check(_lib.load().vissm_feat_fwd(ctypes.byref(d), ctypes.byref(_feat_params(ws)), ptr(h0), ptr(C), ptr(act),
                                     _lib.stream_handle(h0.device)), "vissm_feat_fwd")
    torch.cuda.synchronize()
    return C, act


@pytest.mark.parametrize("n_win,Lh,Cin,H,k,s", [
    (3, 67, 14, 50, 20, 1), (3, 67, 14, 50, 20, 2), (1, 33, 63, 64, 64, 2), (3, 35, 3, 7, 2, 2), (1, 17, 3, 7, 1, 1),
    (3, 1, 14, 50, 5, 1)])
def test_forward_act_rows_and_bitwise_across_variants(monkeypatch, n_win, Lh, Cin, H, k, s):
    """C and all four layers' rows < Lu = s (Lh - 1) + k against float64; rows from Lu on are not written; and the
    three variants agree bit for bit on C and on every act row"""
    h0, ws, dC, ref = _make(n_win, Lh, Cin, H, k, s)
    Cr, acts, _ = ref
    Lu = s * (Lh - 1) + k
    outs = {}
    for kt in KTS:
        _force(monkeypatch, kt, None)
        assert _lib.feat_geometry(_desc(h0, ws, s, Lh), False)["kt"] == kt
        C, act = _fwd_direct(h0, ws, s, Lh)
        assert bool(torch.isfinite(C).all()) and bool(torch.isfinite(act[:, :, :Lu]).all()), kt
        assert bool(torch.isnan(act[:, :, Lu:]).all()), kt          # rows no output reads: left alone
        worst = max(R.rel_l2(C, Cr) / 2e-6, R.max_rel_scale(C, Cr) / 1e-4)
        for l in range(4):
            a, b = act[l, :, :Lu], acts[l][:, :Lu]
            e2, em = R.rel_l2(a, b), R.max_rel_scale(a, b)
            assert e2 < 2e-6 and em <= 1e-4, (kt, l, e2, em)
            worst = max(worst, e2 / 2e-6, em / 1e-4)
        assert worst < 1.0, (kt, worst)
        WORST["act"] = max(WORST.get("act", 0.0), worst)
        outs[kt] = (C, act[:, :, :Lu].clone())
    print(f"[feat-variants] act {(n_win, Lh, Cin, H, k, s)}: group worst error / bar {WORST['act']:.3f}")
    for kt in (16, 32):
        assert torch.equal(outs[8][0], outs[kt][0]), ("C differs between kT 8 and", kt)
        for l in range(4):
            assert torch.equal(outs[8][1][l], outs[kt][1][l]), ("act layer", l, "differs between kT 8 and", kt)
