"""Each stage kernel of the LV / SV feature branch at the C ABI, per element, against tests/feat_ref.py:

* vissm_lv_pack, vissm_lv_conv_wscatter, vissm_lv_conv_diag_bwd (dG): data movement plus round-to-nearest-even bf16
  rounding, held bit for bit, padding and zeros included (the outputs start as NaN: an unwritten element shows);
* vissm_lv_conv_diag: adds only, bit for bit against the sequential fp32 sum started at conv_b[h], j ascending;
* dconv_b: within Lh 2^-23 sum_m |dC[m][h]| of the float64 column sum, the worst case of an fp32 sum in any order;
* vissm_lv_mlp_fwd / _bwd: fp32 FMAs, at the fused branch's bars (relative L2 below 2e-6, every element within 1e-4 of
  the tensor's largest magnitude); the bf16 planes of the last layer bit for bit from the kernel's own fp32 output;
* lv_feat_conv with two windows (the per-window loop, the plane views and the sum over windows of LvFeatConvFn), at
  the bars tests/test_gpu_lvfeat.py holds one window to; sv_feat_conv and lv_feat_conv on views whose windows lie
  further apart than their rows (the descriptors' in_win_stride above its minimum).

In the ops.py chain these kernels are only seen through norm-relative bars over the whole branch, where one wrong
element of a 300,000-element gradient passes."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import feat_ref as R  # noqa: E402
from viforssms_amd import _lib  # noqa: E402
from viforssms_amd._lib import check, ptr  # noqa: E402
from viforssms_amd.ops import lv_feat_conv  # noqa: E402
from viforssms_amd.linalg import linear, linear_bf16  # noqa: E402

DEV = "cuda:0"
BF = torch.bfloat16
NAN = float("nan")
WORST = {}


def _note(group, ratio):
    WORST[group] = max(WORST.get(group, 0.0), float(ratio))
    print(f"[lvfeat-stages] {group}: error / bound {float(ratio):.3f} (group worst {WORST[group]:.3f})")


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _st():
    return _lib.stream_handle(torch.device(DEV))


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def _same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = int((g != w).sum())
    assert bad == 0, f"{what}: {bad} of {g.numel()} elements differ"


# ---------------------------------------------------------------------------------------
# vissm_lv_pack
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo", [False, True])
@pytest.mark.parametrize("H,U,ldw,R_,k,ldc", [
    (50, 61, 64, 70, 9, 450),      # the minimum leading dimensions (ldw = U rounded to 8, ldc = k H)
    (50, 61, 77, 70, 9, 461),      # both above it, odd
    (7, 5, 5, 1, 1, 7),            # ldw = U, one channel, one tap
    (63, 33, 40, 33, 3, 200),      # H = 63: the bias in the last row of W3b
    (50, 0, 0, 50, 20, 1000),      # SV's form: no time-mixing layer (ldw = 0, null w3 / b3 / W3b)
    (12, 0, 0, 12, 5, 67),
])
def test_lv_pack_bitwise(H, U, ldw, R_, k, ldc, lo):
    g = _gen(H + U + R_ + k)
    cw = torch.randn(k, 1 + R_, H, generator=g, device=DEV)
    w3 = torch.randn(H, U, generator=g, device=DEV) if ldw else None
    b3 = torch.randn(U, generator=g, device=DEV) if ldw else None
    nan = lambda *sh: torch.full(sh, NAN, device=DEV, dtype=BF)
    W3b = nan(64, ldw) if ldw else None
    W3lo = nan(64, ldw) if ldw and lo else None
    Wc, Wclo = nan(R_, ldc), (nan(R_, ldc) if lo else None)
    check(_lib.load().vissm_lv_pack(ptr(w3), ptr(b3), H, U, ldw, ptr(W3b), ptr(W3lo), ptr(cw), R_, k, ldc, ptr(Wc),
                                    ptr(Wclo), _st()), "vissm_lv_pack")
    torch.cuda.synchronize()
    want = R.pack_wc(cw.cpu(), R_, k, H, ldc)
    hi, lo_ = R.split_bf16(want)
    _same_bits(Wc, hi, "Wc")
    assert int(torch.count_nonzero(Wc[:, k * H:].float())) == 0
    if lo:
        _same_bits(Wclo, lo_, "Wc lo")
    if ldw:
        want = R.pack_w3b(w3.cpu(), b3.cpu(), H, U, ldw)
        hi, lo_ = R.split_bf16(want)
        _same_bits(W3b, hi, "W3b")
        _same_bits(W3b[H, :U], b3.to(BF), "W3b bias row")
        assert int(torch.count_nonzero(W3b[H + 1:].float())) == 0 and int(torch.count_nonzero(W3b[:, U:].float())) == 0
        if lo:
            _same_bits(W3lo, lo_, "W3b lo")


# ---------------------------------------------------------------------------------------
# vissm_lv_conv_wscatter
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("R_,k,H,ldc", [(70, 9, 50, 456), (1, 1, 7, 7), (33, 3, 63, 195), (50, 20, 50, 1000)])
def test_lv_wscatter_bitwise(R_, k, H, ldc):
    dWc = torch.full((R_, ldc), NAN, device=DEV)
    dWc[:, :k * H] = torch.randn(R_, k * H, generator=_gen(R_ + k), device=DEV)   # the padding is never read
    out = torch.full((k, 1 + R_, H), NAN, device=DEV)
    check(_lib.load().vissm_lv_conv_wscatter(ptr(dWc), ldc, R_, k, H, ptr(out), _st()), "vissm_lv_conv_wscatter")
    torch.cuda.synchronize()
    _same_bits(out, R.wscatter(dWc.cpu(), R_, k, H), "dconv_w")
    assert int(torch.count_nonzero(out[:, 0, :])) == 0


# ---------------------------------------------------------------------------------------
# vissm_lv_conv_diag_bwd / vissm_lv_conv_diag
# ---------------------------------------------------------------------------------------
DIAG = [  # H, k, s, Lh, rows past the last tap, columns past k H
    (50, 9, 1, 1, 0, 0), (50, 9, 2, 1, 3, 6), (50, 9, 1, 255, 2, 6), (50, 9, 2, 255, 0, 0), (50, 9, 1, 256, 0, 6),
    (50, 9, 2, 256, 5, 6), (50, 9, 1, 257, 1, 0), (50, 9, 2, 257, 4, 14), (7, 1, 2, 33, 2, 1), (63, 20, 2, 40, 3, 20),
]


@pytest.mark.parametrize("lo", [False, True])
@pytest.mark.parametrize("H,k,s,Lh,du,dl", DIAG)
def test_lv_diag_bwd_bitwise_and_bias_sum(H, k, s, Lh, du, dl, lo):
    U, ldg = s * (Lh - 1) + k + du, k * H + dl
    dC = torch.randn(Lh, H, generator=_gen(H + k + Lh + s), device=DEV)
    dG = torch.full((U, ldg), NAN, device=DEV, dtype=BF)
    dGlo = torch.full((U, ldg), NAN, device=DEV, dtype=BF) if lo else None
    db = torch.full((H,), NAN, device=DEV)
    check(_lib.load().vissm_lv_conv_diag_bwd(ptr(dC), H, k, s, Lh, U, ldg, ptr(dG), ptr(dGlo), ptr(db), _st()),
          "vissm_lv_conv_diag_bwd")
    torch.cuda.synchronize()
    want, _ = R.diag_bwd(dC.cpu(), H, k, s, Lh, U, ldg)
    hi, lo_ = R.split_bf16(want)
    _same_bits(dG, hi, "dG")
    if lo:
        _same_bits(dGlo, lo_, "dG lo")
    # exactly Lh k H taps are set (random values: none rounds to zero), zeros past k H and past the last tap's row
    assert int(torch.count_nonzero(dG.float())) == Lh * k * H
    assert int(torch.count_nonzero(dG[:, k * H:].float())) == 0
    assert int(torch.count_nonzero(dG[s * (Lh - 1) + k:].float())) == 0
    ref = dC.double().sum(0).cpu()
    bound = Lh * 2.0 ** -23 * dC.double().abs().sum(0).cpu()
    err = (db.double().cpu() - ref).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    _note("dconv_b", (err / bound).max())


@pytest.mark.parametrize("H,k,s,Lh,du,dl", DIAG)
def test_lv_diag_bitwise(H, k, s, Lh, du, dl):
    U, ldg = s * (Lh - 1) + k + du, k * H + dl
    g = _gen(H + k + Lh + s + 1)
    G = torch.full((U, ldg), NAN, device=DEV)       # rows past the last tap and columns past k H are never read
    G[:s * (Lh - 1) + k, :k * H] = torch.randn(s * (Lh - 1) + k, k * H, generator=g, device=DEV)
    cb = torch.randn(H, generator=g, device=DEV)
    C = torch.full((Lh, H), NAN, device=DEV)
    check(_lib.load().vissm_lv_conv_diag(ptr(G), ldg, ptr(cb), H, k, s, Lh, ptr(C), _st()), "vissm_lv_conv_diag")
    torch.cuda.synchronize()
    want = R.diag_f32_sequential(G.cpu().numpy(), cb.cpu().numpy(), H, k, s, Lh)
    _same_bits(C, torch.from_numpy(want), "C")


# ---------------------------------------------------------------------------------------
# vissm_lv_mlp_fwd / _bwd
# ---------------------------------------------------------------------------------------
MLP = [  # n_layers, sv_diff, R, n_win, H, Cin
    (3, 0, 1, 1, 7, 3), (3, 0, 31, 3, 50, 13), (3, 0, 32, 1, 63, 63), (3, 0, 33, 3, 50, 13), (3, 0, 89, 3, 63, 63),
    (4, 1, 1, 3, 50, 14), (4, 1, 31, 1, 63, 62), (4, 1, 32, 3, 7, 2), (4, 1, 33, 1, 50, 14), (4, 1, 89, 3, 63, 62),
    (4, 0, 33, 3, 50, 63), (3, 1, 89, 1, 7, 14),
]
_mlp_cache = {}


def _mlp_case(nl, diff, R_, n_win, H, Cin):
    key = (nl, diff, R_, n_win, H, Cin)
    if key not in _mlp_cache:
        g = _gen(100 * R_ + H + Cin + nl + diff)
        r = lambda *sh, sc=1.0: torch.randn(*sh, generator=g, device=DEV) * sc
        rows, cols = (R_ + 1, (Cin + 2) // 2) if diff else (R_, Cin)
        big = r(n_win, rows * cols + 5)               # windows 5 floats further apart than their rows
        h0 = big[:, :rows * cols].unflatten(1, (rows, cols))
        ws = [r(Cin, H, sc=Cin ** -0.5), r(H, sc=0.1)]
        for _ in range(nl - 1):
            ws += [r(H, H, sc=H ** -0.5), r(H, sc=0.1)]
        dH = r(n_win, R_, H)
        acts, grads = R.lv_mlp_grads(h0, ws, nl, bool(diff), dH)
        d = _lib.LvFeatDesc(n_win, R_, Cin, H, rows * cols + 5, nl, diff)
        _mlp_cache[key] = (h0, big, ws, dH, d, acts, grads)
    return _mlp_cache[key]


def _mlp_params(ts, nl, cls):
    w = [ptr(ts[2 * l]) if l < nl else None for l in range(4)]
    b = [ptr(ts[2 * l + 1]) if l < nl else None for l in range(4)]
    return cls((ctypes.c_void_p * 4)(*w), (ctypes.c_void_p * 4)(*b), None, None)


def _mlp_fwd(case, lo=True):
    h0, big, ws, dH, d, acts, grads = case
    nl, n_win, R_, H = d.n_layers, d.n_win, d.R, d.H
    act = torch.full((nl, n_win, R_, H), NAN, device=DEV)
    H3b = torch.full((n_win, R_, 64), NAN, device=DEV, dtype=BF)
    H3lo = torch.full((n_win, R_, 64), NAN, device=DEV, dtype=BF) if lo else None
    check(_lib.load().vissm_lv_mlp_fwd(ctypes.byref(d), ctypes.byref(_mlp_params(ws, nl, _lib.FeatParams)), ptr(big),
                                       ptr(act), ptr(H3b), ptr(H3lo), _st()), "vissm_lv_mlp_fwd")
    torch.cuda.synchronize()
    return act, H3b, H3lo


@pytest.mark.parametrize("nl,diff,R_,n_win,H,Cin", MLP)
def test_lv_mlp_fwd(nl, diff, R_, n_win, H, Cin):
    case = _mlp_case(nl, diff, R_, n_win, H, Cin)
    acts = case[5]
    act, H3b, H3lo = _mlp_fwd(case)
    worst = 0.0
    for l in range(nl):
        e2, em = R.rel_l2(act[l], acts[l]), R.max_rel_scale(act[l], acts[l])
        assert e2 < 2e-6 and em <= 1e-4, (l, e2, em)
        worst = max(worst, e2 / 2e-6, em / 1e-4)
    _note("mlp_fwd act", worst)
    last = act[nl - 1]
    hi = last.to(BF)
    _same_bits(H3b[..., :H], hi, "H3b")
    _same_bits(H3lo[..., :H], (last - hi.float()).to(BF), "H3lo")
    assert bool((H3b[..., H].float() == 1.0).all())                      # the ones column (W3b's bias row)
    assert int(torch.count_nonzero(H3b[..., H + 1:].float())) == 0
    assert int(torch.count_nonzero(H3lo[..., H:].float())) == 0 and bool(torch.isfinite(H3lo.float()).all())
    # without the residual plane: the same hi plane
    _, H3b1, _ = _mlp_fwd(case, lo=False)
    _same_bits(H3b1, H3b, "H3b without the lo plane")


@pytest.mark.parametrize("ld64", [False, True])
@pytest.mark.parametrize("nl,diff,R_,n_win,H,Cin", MLP)
def test_lv_mlp_bwd(nl, diff, R_, n_win, H, Cin, ld64):
    case = _mlp_case(nl, diff, R_, n_win, H, Cin)
    h0, big, ws, dH, d, acts, grads = case
    act, _, _ = _mlp_fwd(case, lo=False)
    ld = 64 if ld64 else H
    dH3 = torch.full((n_win, R_, ld), NAN, device=DEV)     # columns >= H are never read
    dH3[..., :H] = dH
    gr = [torch.full_like(w, NAN) for w in ws]
    lib = _lib.load()
    nb = lib.vissm_lv_mlp_workspace_size(ctypes.byref(d))
    assert nb > 0
    wsb = torch.empty(nb, dtype=torch.uint8, device=DEV)
    check(lib.vissm_lv_mlp_bwd(ctypes.byref(d), ctypes.byref(_mlp_params(ws, nl, _lib.FeatParams)), ptr(big), ptr(act),
                               ptr(dH3), ld, ctypes.byref(_mlp_params(gr, nl, _lib.FeatGrads)), ptr(wsb), nb, _st()),
          "vissm_lv_mlp_bwd")
    torch.cuda.synchronize()
    worst = 0.0
    for i, (a, b) in enumerate(zip(gr, grads)):
        assert bool(torch.isfinite(a).all()), i
        e2, em = R.rel_l2(a, b), R.max_rel_scale(a, b)
        assert e2 < 2e-6 and em <= 1e-4, (i, e2, em)
        worst = max(worst, e2 / 2e-6, em / 1e-4)
    _note("mlp_bwd grads", worst)


# ---------------------------------------------------------------------------------------
# SV with windows further apart than their rows
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2])
def test_sv_feat_conv_windows_apart(s):
    """sv_feat_conv on a view whose windows lie further apart than L Cr (in_win_stride above its minimum through
    SvFeatConvFn), against float64, at tests/test_gpu_svfeat.py's bars: 3x the fp32 torch form's error + 2e-5"""
    from tests.test_gpu_svfeat import _torch_form
    from viforssms_amd.ops import sv_feat_conv
    L, Cr, k, H = 71, 5, 9, 50
    Cin = 2 * Cr - 2
    g = _gen(71 + s)
    r = lambda *sh, sc=1.0: (torch.randn(*sh, generator=g, device=DEV) * sc).requires_grad_(True)
    ws = [r(Cin, H, sc=0.3), r(H, sc=0.1), r(H, H, sc=0.15), r(H, sc=0.1), r(H, H, sc=0.15), r(H, sc=0.1),
          r(H, H, sc=0.15), r(H, sc=0.1), r(k, 1 + H, H, sc=0.03), r(H, sc=0.1)]
    ts = torch.randn(2, L + 3, Cr, generator=g, device=DEV)[:, 2:2 + L, :]
    Lh = (L - 1 - k) // s + 1
    dC = torch.randn(2, Lh, H, generator=g, device=DEV)
    wd = [R.to64(w).requires_grad_(True) for w in ws]
    C64 = R.sv_branch_staged(R.to64(ts), wd, s, Lh)
    g64 = torch.autograd.grad(C64, wd, R.to64(dC))
    Ch = sv_feat_conv(ts, s, Lh, *ws)
    gh = torch.autograd.grad(Ch, ws, dC)
    Ct = _torch_form(ts.contiguous(), ws, s, Lh)
    gt = torch.autograd.grad(Ct, ws, dC)
    e_h, e_t = R.rel_l2(Ch, C64), R.rel_l2(Ct, C64)
    assert e_h < 3 * e_t + 2e-5, ("C", e_h, e_t)
    worst = e_h / (3 * e_t + 2e-5)
    for i, (a, b, ref) in enumerate(zip(gh, gt, g64)):
        if i == 8:
            assert float(a[:, 0, :].abs().max()) == 0.0
        e_h, e_t = R.rel_l2(a, ref), R.rel_l2(b, ref)
        assert e_h < 3 * e_t + 2e-5, (i, e_h, e_t)
        worst = max(worst, e_h / (3 * e_t + 2e-5))
    _note("sv windows apart", worst)


# ---------------------------------------------------------------------------------------
# LV with several windows
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("x3", [False, True])
@pytest.mark.parametrize("s", [1, 2])
def test_lv_feat_conv_two_windows(s, x3):
    """C and every gradient at n_win = 2 against float64 (tests/feat_ref.py's staged form), held to one window's bars
    of tests/test_gpu_lvfeat.py: within 3x the torch form's own error (bf16: the linear_bf16 form, + 1e-3 at C and
    2e-3 at the gradients; x3: the fp32 form, + 2e-5)"""
    from tests.test_gpu_lvfeat import _torch_form
    R_, U, k, Cin, H = 70, 61, 9, 13, 50
    g = _gen(70 + 61 + s)
    r = lambda *sh, sc=1.0: (torch.randn(*sh, generator=g, device=DEV) * sc).requires_grad_(True)
    ws = [r(Cin, H, sc=0.3), r(H, sc=0.1), r(H, H, sc=0.15), r(H, sc=0.1), r(H, H, sc=0.15), r(H, sc=0.1),
          r(H, U, sc=0.15), r(U, sc=0.1), r(k, 1 + R_, H, sc=0.02), r(H, sc=0.1)]
    big = torch.randn(2, R_ + 3, Cin, generator=g, device=DEV)
    h0 = big[:, 1:1 + R_, :]                      # windows further apart than R Cin
    Lh = (U - k) // s + 1
    dC = torch.randn(2, Lh, H, generator=g, device=DEV)

    def grads(fn):
        C = fn()
        return C.detach(), torch.autograd.grad(C, ws, dC)

    wd = [R.to64(w).requires_grad_(True) for w in ws]
    C64 = R.lv_branch_staged(R.to64(h0), wd, s, Lh)
    g64 = torch.autograd.grad(C64, wd, R.to64(dC))
    lin = linear if x3 else linear_bf16
    fa, fg = (2e-5, 2e-5) if x3 else (1e-3, 2e-3)
    Ch, gh = grads(lambda: lv_feat_conv(h0, s, Lh, *ws, x3=x3))
    hc = h0.contiguous()                          # (the torch form takes one window at a time)
    Ct, gt = grads(lambda: torch.cat([_torch_form(hc[w:w + 1], ws, s, Lh, lin) for w in range(2)]))
    assert Ch.shape == (2, Lh, H)
    e_h, e_t = R.rel_l2(Ch, C64), R.rel_l2(Ct, C64)
    assert e_h < 3 * e_t + fa, ("C", e_h, e_t)
    worst = e_h / (3 * e_t + fa)
    # each window's C on its own (a plane view off by one window would still pass a norm over both)
    for w in range(2):
        e_w, e_tw = R.rel_l2(Ch[w], C64[w]), R.rel_l2(Ct[w], C64[w])
        assert e_w < 3 * e_tw + fa, ("C window", w, e_w, e_tw)
    for i, (a, b, ref) in enumerate(zip(gh, gt, g64)):
        if i == 8:
            assert float(a[:, 0, :].abs().max()) == 0.0
        e_h, e_t = R.rel_l2(a, ref), R.rel_l2(b, ref)
        assert e_h < 3 * e_t + fg, (i, e_h, e_t)
        worst = max(worst, e_h / (3 * e_t + fg))
    _note(f"lv two windows x3={x3}", worst)
