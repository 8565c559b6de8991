"""torch.autograd wrappers around the libvissm HIP kernels.

Each Function's forward and backward is exactly one C-ABI call (plus
caller-allocated workspace from torch's caching allocator, so no hipMalloc
happens on the step path).  Tensors must be contiguous fp32 on the current
HIP device.
"""
from __future__ import annotations

import ctypes
import os
import dataclasses
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from ._lib import FlowDesc, FlowParams, FlowGrads, ElboDesc, ElboData, GatherDesc, check, ptr


_FORCE_DU = os.environ.get("VISSM_FORCE_DU") == "1"  # A/B timing hook: always compute the flows' du


def _require_gpu(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.VissmError("libvissm kernels run on the GPU only; got a CPU tensor "
                                  "(there is deliberately no CPU fallback)")
        if t.dtype not in (torch.float32, torch.int32):
            raise _lib.VissmError(f"expected fp32/int32 tensors, got {t.dtype}")
        if not t.is_contiguous():
            raise _lib.VissmError("expected contiguous tensors")


def _require_rows(*ts):
    """As _require_gpu for [B, n] row tensors that may lie a pitch apart (VissmFlowDesc.u_pitch / out_pitch)."""
    for t in ts:
        _require_gpu(t[0] if t.dim() == 2 and t.stride(1) == 1 else t)   # one row: unit stride


def _workspace(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


# ---------------------------------------------------------------------------------------
# base noise
# ---------------------------------------------------------------------------------------
def normal_base(seed: int, offset: int, B: int, L: int, n_last: int, device) -> (torch.Tensor, torch.Tensor):
    """init_dist.slp (AR.py:31-35): eps ~ N(0,1) [B, L] and the base log-prob over the last n_last entries."""
    lib = _lib.load()
    eps = torch.empty(B, L, dtype=torch.float32, device=device)
    lp = torch.empty(B, dtype=torch.float32, device=device)
    check(lib.vissm_normal_base(ctypes.c_uint64(seed & (2 ** 64 - 1)), ctypes.c_uint64(offset), ptr(eps), ptr(lp),
                                B, L, n_last, _lib.stream_handle(device)), "vissm_normal_base")
    return eps, lp


def normal_base_dev(seed: int, offset_dev: torch.Tensor, B: int, L: int, n_last: int):
    """normal_base with the Philox row offset in a device uint64 (int64 storage) tensor."""
    lib = _lib.load()
    if not (offset_dev.is_cuda and offset_dev.dtype == torch.int64 and offset_dev.numel() == 1):
        raise _lib.VissmError("normal_base_dev: offset must be one int64 on the GPU")
    dev = offset_dev.device
    eps = torch.empty(B, L, dtype=torch.float32, device=dev)
    lp = torch.empty(B, dtype=torch.float32, device=dev)
    check(lib.vissm_normal_base_dev(ctypes.c_uint64(seed & (2 ** 64 - 1)), ptr(offset_dev), ptr(eps), ptr(lp),
                                    B, L, n_last, _lib.stream_handle(dev)), "vissm_normal_base_dev")
    return eps, lp


def base_logprob(eps: torch.Tensor, n_last: int) -> torch.Tensor:
    lib = _lib.load()
    _require_gpu(eps)
    B, L = eps.shape
    lp = torch.empty(B, dtype=torch.float32, device=eps.device)
    check(lib.vissm_base_logprob(ptr(eps), ptr(lp), B, L, n_last, _lib.stream_handle(eps.device)),
          "vissm_base_logprob")
    return lp


# ---------------------------------------------------------------------------------------
# split-bf16 operand planes
# ---------------------------------------------------------------------------------------
def _dense_layout(t: torch.Tensor) -> bool:
    """t covers its storage span densely in some dimension order (a contiguous tensor or a permuted view of one)."""
    dims = sorted((st, sz) for st, sz in zip(t.stride(), t.shape) if sz > 1)
    expect = 1
    for st, sz in dims:
        if st != expect:
            return False
        expect *= sz
    return True


def theta_branch_fwd(theta, W0, b0, W1, b1, W2, b2, term: bool = True):
    """The flows' theta-branch forward (include/vissm.h vissm_theta_branch_fwd; nma._ThetaBranchK): the collapsed
    weights (Wc, bc) and, if term, theta_term = theta Wc + bc -- (theta_term or None, Wc, bc)."""
    lib = _lib.load()
    _require_gpu(W0, b0, W1, b1, W2, b2)
    P, n0 = W0.shape
    n1, H = W1.shape[1], W2.shape[1]
    dev = W0.device
    ws = [t.contiguous().float() for t in (W0, b0, W1, b1, W2, b2)]
    Wc, bc = torch.empty(P, H, device=dev), torch.empty(H, device=dev)
    tt, th, B = None, None, 0
    if term:
        th = theta.contiguous().float()
        B = th.shape[0]
        tt = torch.empty(B, H, device=dev)
    check(lib.vissm_theta_branch_fwd(B, P, n0, n1, H, ptr(th), *[ptr(t) for t in ws], ptr(Wc), ptr(bc), ptr(tt),
                                     _lib.stream_handle(dev)), "vissm_theta_branch_fwd")
    return tt, Wc, bc


def theta_branch_bwd(theta, d, W0, b0, W1, b1, W2):
    """The flows' theta-branch backward (include/vissm.h vissm_theta_branch_bwd; nma._ThetaBranch): dtheta and the
    gradients of (W0, b0, W1, b1, W2, b2) from d = d loss / d theta_term, in three launches."""
    lib = _lib.load()
    _require_gpu(theta, d, W0, b0, W1, b1, W2)
    B, P = theta.shape
    n0, n1, H = W0.shape[1], W1.shape[1], W2.shape[1]
    dev = d.device
    args = [t.contiguous().float() for t in (theta, d, W0, b0, W1, b1, W2)]
    outs = [torch.empty(sh, device=dev) for sh in ((B, P), (P, n0), (n0,), (n0, n1), (n1,), (n1, H), (H,))]
    nb = lib.vissm_theta_branch_bwd_workspace_size(B, P)
    ws = _workspace(nb, dev)
    check(lib.vissm_theta_branch_bwd(B, P, n0, n1, H, *[ptr(t) for t in args], *[ptr(t) for t in outs], ptr(ws), nb,
                                     _lib.stream_handle(dev)), "vissm_theta_branch_bwd")
    return tuple(outs)


def split_bf16(x: torch.Tensor):
    """(hi, lo) bf16 planes with x = hi + lo to ~2^-16 relative (vissm_split_bf16, one pass over x), laid out with
    x's strides: x may be a transposed view (LV's time-mixing features)."""
    if not x.is_cuda or x.dtype != torch.float32:
        raise _lib.VissmError("split_bf16: fp32 GPU tensor expected (there is deliberately no CPU fallback)")
    if not _dense_layout(x):
        x = x.contiguous()
    hi = torch.empty_strided(x.shape, x.stride(), dtype=torch.bfloat16, device=x.device)
    lo = torch.empty_strided(x.shape, x.stride(), dtype=torch.bfloat16, device=x.device)
    if x.data_ptr() % 16:
        x = x.clone(memory_format=torch.preserve_format)
    check(_lib.load().vissm_split_bf16(ptr(x), ptr(hi), ptr(lo), x.numel(), _lib.stream_handle(x.device)),
          "vissm_split_bf16")
    return hi, lo


# ---------------------------------------------------------------------------------------
# window gather
# ---------------------------------------------------------------------------------------
def gather_windows(src: torch.Tensor, starts: torch.Tensor, out: torch.Tensor, n: int, length: int, C: int,
                   stride: int = 1, offset: int = 0, j_step: int = 1, c_pitch: int = 0, os=None) -> torch.Tensor:
    """out[r*os_r + j*os_j + c*os_c] = src.flat[c*c_pitch + stride*starts[r] + offset + j*j_step]
    (vissm_gather_windows: the train loop's window gather, AR.py:267-288, from a device-resident table)."""
    _require_gpu(src, starts, out)
    if starts.dtype != torch.int32 or src.dtype != torch.float32:
        raise _lib.VissmError("gather_windows: int32 starts and fp32 tables expected")
    os_r, os_j, os_c = os
    d = GatherDesc(n, length, C, stride, offset, j_step, c_pitch, os_r, os_j, os_c)
    check(_lib.load().vissm_gather_windows(ctypes.byref(d), ptr(src), ptr(starts), ptr(out),
                                           _lib.stream_handle(src.device)), "vissm_gather_windows")
    return out


# ---------------------------------------------------------------------------------------
# IAF flow
# ---------------------------------------------------------------------------------------
@dataclass(frozen=True)
class FlowShape:
    B: int
    L: int
    k: int
    H: int
    n_hidden: int
    bn: bool
    stride2: bool
    swap_out: bool
    n_logsig: int
    n_win: int
    precision: int = _lib.VISSM_PREC_FP32
    bwd_precision: Optional[int] = None   # the backward kernel's precision when it differs (VISSM_PREC_BF16X3F)
    chunk_tiles: int = 0                  # VissmFlowDesc.chunk_tiles: 0 = automatic launch geometry
    pad_out: bool = False                 # u_next rows padded to 16 floats (it feeds another flow, whose du stores
                                          # are then 64-byte aligned)

    def desc(self, u_pitch: int = 0, out_pitch: int = 0) -> FlowDesc:
        return FlowDesc(self.B, self.L, self.k, self.H, self.n_hidden, int(self.bn), int(self.stride2),
                        int(self.swap_out), self.n_logsig, self.n_win, self.precision, int(self.chunk_tiles),
                        int(u_pitch), int(out_pitch))

    @property
    def Lout(self):
        return self.L - self.k

    @property
    def Lh(self):
        return self.Lout // (2 if self.stride2 else 1)


def kernel_precision(shape: FlowShape) -> int:
    """vissm_flow_kernel_precision: the precision the flow kernels compute `shape` in (its own, or fp32 where the
    matrix-core kernels do not cover it)."""
    rc = _lib.load().vissm_flow_kernel_precision(ctypes.byref(shape.desc()))
    if rc < 0:
        check(rc, "vissm_flow_kernel_precision")
    return rc


def _flow_params(w_eps, w_hid, b_hid, bn_g, bn_b, w_head, b_head, tf=None) -> FlowParams:
    """VissmFlowParams; tf = (theta [B, R], w_theta [R, H], b_theta [H]) is the theta branch's factorization
    (theta_term = theta w_theta + b_theta), which the two-sample AR kernels fold into their layer-0 product."""
    if tf is None:
        return FlowParams(ptr(w_eps), ptr(w_hid), ptr(b_hid), ptr(bn_g), ptr(bn_b), ptr(w_head), ptr(b_head))
    th, wt, bt = tf
    _require_gpu(th, wt, bt)
    if not (th.is_contiguous() and wt.is_contiguous() and bt.is_contiguous()) or th.shape[1] != wt.shape[0]:
        raise _lib.VissmError("theta factors: contiguous theta [B, R], w_theta [R, H], b_theta [H] expected")
    return FlowParams(ptr(w_eps), ptr(w_hid), ptr(b_hid), ptr(bn_g), ptr(bn_b), ptr(w_head), ptr(b_head),
                      ptr(th), ptr(wt), ptr(bt), int(th.shape[1]))


# ---------------------------------------------------------------------------------------
# window-shared feature branch + the first conv's feature channels (vissm_feat_fwd / _bwd)
# ---------------------------------------------------------------------------------------
class FeatConvFn(torch.autograd.Function):
    """C [n_win, Lh, H] = conv_b + the feature channels of the first conv over F = the four dense + ELU layers
    of the window's time features h0 [n_win, Lf, Cin] (AR.py:53-62; SV_dense.py:53-62; fitz_nag_NVP.py:71-79), one
    HIP launch each way (the torch form is ~40 small launches per flow).  The gradient reaches the four dense
    layers and the conv kernel (its sample channel 0 gets zero here: that part is the flow kernel's w_eps) and
    bias; h0 is data."""

    @staticmethod
    def forward(ctx, h0, s, Lh, W0, b0, W1, b1, W2, b2, W3, b3, conv_w, conv_b):
        ws = (W0, b0, W1, b1, W2, b2, W3, b3, conv_w, conv_b)
        _require_gpu(*ws)
        n_win, Lf, Cin = h0.shape
        if not h0.is_cuda or h0.dtype != torch.float32 or h0.stride(2) != 1 or h0.stride(1) != Cin:
            h0 = h0.contiguous()
            _require_gpu(h0)
        H, k = W3.shape[1], conv_w.shape[0]
        d = _lib.FeatDesc(n_win, Lf, Cin, H, k, s, Lh, h0.stride(0) if n_win > 1 else Lf * Cin)
        p = _feat_params(ws)
        C = torch.empty(n_win, Lh, H, dtype=torch.float32, device=h0.device)
        act = torch.empty(4, n_win, Lf, H, dtype=torch.float32, device=h0.device)
        check(_lib.load().vissm_feat_fwd(ctypes.byref(d), ctypes.byref(p), ptr(h0), ptr(C), ptr(act),
                                         _lib.stream_handle(h0.device)), "vissm_feat_fwd")
        ctx.save_for_backward(h0, act, *ws)
        ctx.desc = d
        return C

    @staticmethod
    def backward(ctx, dC):
        h0, act, *ws = ctx.saved_tensors
        d = ctx.desc
        dC = dC.contiguous()
        gr = [torch.empty_like(t) for t in ws]
        g = _lib.FeatGrads((ctypes.c_void_p * 4)(*[ptr(t) for t in gr[0:8:2]]),
                           (ctypes.c_void_p * 4)(*[ptr(t) for t in gr[1:8:2]]), ptr(gr[8]), ptr(gr[9]))
        lib = _lib.load()
        nb = lib.vissm_feat_workspace_size(ctypes.byref(d))
        if nb == 0:
            raise _lib.VissmError(f"vissm_feat_workspace_size failed: {lib.vissm_last_error().decode()}")
        wsb = _workspace(nb, dC.device)
        check(lib.vissm_feat_bwd(ctypes.byref(d), ctypes.byref(_feat_params(ws)), ptr(h0), ptr(act), ptr(dC),
                                 ctypes.byref(g), ptr(wsb), nb, _lib.stream_handle(dC.device)), "vissm_feat_bwd")
        return (None, None, None, *gr)


def _feat_params(ws) -> "_lib.FeatParams":
    return _lib.FeatParams((ctypes.c_void_p * 4)(*[ptr(t) for t in ws[0:8:2]]),
                           (ctypes.c_void_p * 4)(*[ptr(t) for t in ws[1:8:2]]), ptr(ws[8]), ptr(ws[9]))


def feat_conv(h0, s: int, Lh: int, W0, b0, W1, b1, W2, b2, W3, b3, conv_w, conv_b):
    return FeatConvFn.apply(h0, s, Lh, W0, b0, W1, b1, W2, b2, W3, b3, conv_w, conv_b)


# ---------------------------------------------------------------------------------------
# bf16 matrix-core GEMM (vissm_gemm_bf16) and Lotka-Volterra's feature branch built on it (vissm_lv_*)
# ---------------------------------------------------------------------------------------
def gemm_bf16(M: int, N: int, K: int, A, lda: int, a_kmajor: bool, B, ldb: int, b_kmajor: bool, C, ldc: int,
              epilogue: int = 0, aux=None, split_k: int = 1):
    """C[m][n] = sum_k A[m][k] B[k][n] on bf16 operands (layouts: include/vissm.h VissmGemmDesc); C fp32 or, for the
    ELU / elu' epilogues, bf16."""
    lib = _lib.load()
    d = _lib.GemmDesc(M, N, K, lda, ldb, ldc, int(a_kmajor), int(b_kmajor), epilogue, split_k)
    nb = lib.vissm_gemm_workspace_size(ctypes.byref(d))
    ws = _workspace(nb, C.device) if nb else None
    check(lib.vissm_gemm_bf16(ctypes.byref(d), ptr(A), ptr(B), ptr(C), ptr(aux) if aux is not None else None,
                              ptr(ws) if ws is not None else None, nb, _lib.stream_handle(C.device)), "vissm_gemm_bf16")


def gemm_bf16x3(M: int, N: int, K: int, A, A_lo, lda: int, a_kmajor: bool, B, B_lo, ldb: int, b_kmajor: bool, C,
                ldc: int, epilogue: int = 0, aux=None, split_k: int = 1):
    """C = A_hi B_hi + A_hi B_lo + A_lo B_hi: the split-bf16 form of gemm_bf16, fp32-class products (fp32 C, or for
    the ELU / elu' epilogues a [2][M][ldc] bf16 hi / lo plane pair, aux the same)"""
    lib = _lib.load()
    d = _lib.GemmDesc(M, N, K, lda, ldb, ldc, int(a_kmajor), int(b_kmajor), epilogue, split_k)
    nb = lib.vissm_gemm_bf16x3_workspace_size(ctypes.byref(d))
    ws = _workspace(nb, C.device) if nb else None
    check(lib.vissm_gemm_bf16x3(ctypes.byref(d), ptr(A), ptr(A_lo), ptr(B), ptr(B_lo), ptr(C),
                                ptr(aux) if aux is not None else None, ptr(ws) if ws is not None else None, nb,
                                _lib.stream_handle(C.device)), "vissm_gemm_bf16x3")


def _r8(n: int) -> int:
    return (n + 7) // 8 * 8


class LvFeatConvFn(torch.autograd.Function):
    """Lotka-Volterra's window-shared conv input C [n_win, Lh, H] (lotka_volterra_partial.py:71-82): the three dense +
    ELU layers of the window's time features h0 [n_win, R, Cin] (fp32, vissm_lv_mlp_*), the time-mixing layer
    D = elu(H3 W3 + b3) [R, U] and the conv over D's R channels (transposed by the reference, U its time axis) as
    matrix-core GEMMs (vissm_gemm_bf16: the layer with its ELU in the epilogue, then G = D^T Wc [U, k H] and the
    conv's diagonal sum), and the backward the same way (dD with elu' in the epilogue, dWc = D dG, dW3 = H3^T dP and
    dH3 = dP W3^T split over K).  x3 = False: the bf16 precision's arithmetic (the torch form: fp32 layers,
    linear_bf16 conv) plus bf16 operands in the time-mixing layer.  x3 = True (the parity precisions): every product
    in the split-bf16 form (vissm_gemm_bf16x3, fp32-class; D and dP kept as hi / lo plane pairs).  The gradient
    reaches the four dense layers and the conv kernel (its sample channel 0 gets zero: the flow kernel's w_eps) and
    bias."""

    @staticmethod
    def _mm(x3, M, N, K, A, lda, akm, B, ldb, bkm, C, ldc, epi=0, aux=None, split=1):
        """C = A B with A / B (hi, lo) pairs: one bf16 product (x3 False: the hi planes) or the split-bf16 form"""
        if x3:
            gemm_bf16x3(M, N, K, A[0], A[1], lda, akm, B[0], B[1], ldb, bkm, C, ldc, epi, aux, split)
        else:
            gemm_bf16(M, N, K, A[0], lda, akm, B[0], ldb, bkm, C, ldc, epi, aux, split)

    @staticmethod
    def forward(ctx, h0, s, Lh, x3, W0, b0, W1, b1, W2, b2, W3, b3, conv_w, conv_b):
        ws = (W0, b0, W1, b1, W2, b2, W3, b3, conv_w, conv_b)
        _require_gpu(*ws)
        n_win, R, Cin = h0.shape
        # windows may lie further apart than R Cin (a view whose rows are contiguous: in_win_stride below)
        if not h0.is_cuda or h0.dtype != torch.float32 or h0.stride(2) != 1 or h0.stride(1) != Cin:
            h0 = h0.contiguous()
            _require_gpu(h0)
        H, U, k = W0.shape[1], W3.shape[1], conv_w.shape[0]
        if tuple(conv_w.shape) != (k, 1 + R, H) or s * (Lh - 1) + k > U or H >= 64:
            raise _lib.VissmError(f"lv_feat: conv_w {tuple(conv_w.shape)}, R {R}, U {U}, Lh {Lh}, s {s}: shapes "
                                  "do not match")
        dev = h0.device
        Up, NC = _r8(U), _r8(k * H)
        npl = 2 if x3 else 1   # bf16 planes per operand
        lib, st = _lib.load(), _lib.stream_handle(dev)
        d = _lib.LvFeatDesc(n_win, R, Cin, H, h0.stride(0) if n_win > 1 else R * Cin, 3, 0)
        p = _feat_params(ws)
        act = torch.empty(3, n_win, R, H, dtype=torch.float32, device=dev)
        H3b = torch.empty(npl, n_win, R, 64, dtype=torch.bfloat16, device=dev)
        check(lib.vissm_lv_mlp_fwd(ctypes.byref(d), ctypes.byref(p), ptr(h0), ptr(act), ptr(H3b[0]),
                                   ptr(H3b[1]) if x3 else None, st), "vissm_lv_mlp_fwd")
        W3b = torch.empty(npl, 64, Up, dtype=torch.bfloat16, device=dev)
        Wc = torch.empty(npl, R, NC, dtype=torch.bfloat16, device=dev)
        check(lib.vissm_lv_pack(ptr(W3), ptr(b3), H, U, Up, ptr(W3b[0]), ptr(W3b[1]) if x3 else None, ptr(conv_w), R,
                                k, NC, ptr(Wc[0]), ptr(Wc[1]) if x3 else None, st), "vissm_lv_pack")
        D = torch.empty(n_win, npl, R, Up, dtype=torch.bfloat16, device=dev)   # hi (/ lo) planes per window
        G = torch.empty(U, NC, dtype=torch.float32, device=dev)
        C = torch.empty(n_win, Lh, H, dtype=torch.float32, device=dev)
        sk = int(os.environ.get("VISSM_LV_SPLIT", "5"))
        mm = LvFeatConvFn._mm
        for w in range(n_win):
            mm(x3, R, U, 64, H3b[:, w], 64, False, W3b, Up, True, D[w], Up, _lib.GEMM_ELU_BF16)
            mm(x3, U, NC, R, D[w], Up, True, Wc, NC, True, G, NC, split=sk)
            check(lib.vissm_lv_conv_diag(ptr(G), NC, ptr(conv_b), H, k, s, Lh, ptr(C[w]), st), "vissm_lv_conv_diag")
        ctx.save_for_backward(h0, act, H3b, D, W3b, Wc, *ws)
        ctx.dims = (d, n_win, R, H, U, k, s, Lh, Up, NC, x3)
        return C

    @staticmethod
    def backward(ctx, dC):
        h0, act, H3b, D, W3b, Wc, *ws = ctx.saved_tensors
        d, n_win, R, H, U, k, s, Lh, Up, NC, x3 = ctx.dims
        dev = dC.device
        dC = dC.contiguous()
        npl = 2 if x3 else 1
        lib, st = _lib.load(), _lib.stream_handle(dev)
        dG = torch.empty(npl, U, NC, dtype=torch.bfloat16, device=dev)
        dP = torch.empty(npl, R, Up, dtype=torch.bfloat16, device=dev)
        dWc = torch.empty(n_win, R, NC, dtype=torch.float32, device=dev)
        dW3b = torch.empty(n_win, 64, U, dtype=torch.float32, device=dev)
        dH3 = torch.empty(n_win, R, 64, dtype=torch.float32, device=dev)
        dcb = torch.empty(n_win, H, dtype=torch.float32, device=dev)
        sk = int(os.environ.get("VISSM_LV_SPLIT", "5"))
        sw = int(os.environ.get("VISSM_LV_SPLIT_W3", "8"))
        mm = LvFeatConvFn._mm
        for w in range(n_win):
            check(lib.vissm_lv_conv_diag_bwd(ptr(dC[w]), H, k, s, Lh, U, NC, ptr(dG[0]), ptr(dG[1]) if x3 else None,
                                             ptr(dcb[w]), st), "vissm_lv_conv_diag_bwd")
            mm(x3, R, U, NC, Wc, NC, False, dG, NC, False, dP, Up, _lib.GEMM_DELU_BF16, aux=D[w])
            mm(x3, R, NC, U, D[w], Up, False, dG, NC, True, dWc[w], NC, split=sk)
            mm(x3, 64, U, R, H3b[:, w], 64, True, dP, Up, True, dW3b[w], U, split=sw)
            mm(x3, R, 64, U, dP, Up, False, W3b, Up, False, dH3[w], 64, split=sw)
        if n_win > 1:   # (the reference's LV windows: one per step at the benchmark shapes)
            dWc, dW3b, dcb = dWc.sum(0, keepdim=True), dW3b.sum(0, keepdim=True), dcb.sum(0, keepdim=True)
        gr = [torch.empty_like(t) for t in ws[:6]]
        dconv_w = torch.empty_like(ws[8])
        check(lib.vissm_lv_conv_wscatter(ptr(dWc[0]), NC, R, k, H, ptr(dconv_w), st), "vissm_lv_conv_wscatter")
        g = _lib.FeatGrads((ctypes.c_void_p * 4)(ptr(gr[0]), ptr(gr[2]), ptr(gr[4]), None),
                           (ctypes.c_void_p * 4)(ptr(gr[1]), ptr(gr[3]), ptr(gr[5]), None), None, None)
        nb = lib.vissm_lv_mlp_workspace_size(ctypes.byref(d))
        if nb == 0:
            raise _lib.VissmError(f"vissm_lv_mlp_workspace_size failed: {lib.vissm_last_error().decode()}")
        wsb = _workspace(nb, dev)
        check(lib.vissm_lv_mlp_bwd(ctypes.byref(d), ctypes.byref(_feat_params(ws)), ptr(h0), ptr(act), ptr(dH3), 64,
                                   ctypes.byref(g), ptr(wsb), nb, st), "vissm_lv_mlp_bwd")
        return (None, None, None, None, *gr, dW3b[0, :H], dW3b[0, H], dconv_w, dcb[0])


def lv_feat_conv(h0, s: int, Lh: int, W0, b0, W1, b1, W2, b2, W3, b3, conv_w, conv_b, x3: bool = False):
    return LvFeatConvFn.apply(h0, s, Lh, bool(x3), W0, b0, W1, b1, W2, b2, W3, b3, conv_w, conv_b)


class SvFeatConvFn(torch.autograd.Function):
    """Stochastic volatility's window-shared conv input C [n_win, Lh, H] (SV_dense.py:50-62): the four dense + ELU
    layers over the window's time features with their first differences (the input assembly inside the kernel:
    vissm_lv_mlp_* at n_layers = 4, sv_diff = 1; fp32), then the conv over the 50 feature channels at kernel_len 50
    as one split-bf16 matrix-core GEMM G = F [Wc_0 | .. | Wc_{k-1}] (vissm_gemm_bf16x3: fp32-class products, the
    torch form's fp32 arithmetic to ~1e-6) and its diagonal sum; backward: dG (hi / lo planes), dF = dG Wc^T and
    dWc = F^T dG the same way, then the four layers' gradients.  ts [n_win, L, Cr] gets no gradient (data)."""

    @staticmethod
    def forward(ctx, ts, s, Lh, W0, b0, W1, b1, W2, b2, W3, b3, conv_w, conv_b):
        ws = (W0, b0, W1, b1, W2, b2, W3, b3, conv_w, conv_b)
        _require_gpu(*ws)
        n_win, L, Cr = ts.shape
        # windows may lie further apart than L Cr (a view whose rows are contiguous: in_win_stride below)
        if not ts.is_cuda or ts.dtype != torch.float32 or ts.stride(2) != 1 or ts.stride(1) != Cr:
            ts = ts.contiguous()
            _require_gpu(ts)
        R, Cin = L - 1, 2 * Cr - 2
        H, k = W0.shape[1], conv_w.shape[0]
        if (tuple(W0.shape) != (Cin, H) or tuple(W3.shape) != (H, H) or tuple(conv_w.shape) != (k, 1 + H, H)
                or s * (Lh - 1) + k > R or H >= 64):
            raise _lib.VissmError(f"sv_feat: ts {tuple(ts.shape)}, W0 {tuple(W0.shape)}, conv_w {tuple(conv_w.shape)}, "
                                  f"Lh {Lh}, s {s}: shapes do not match")
        dev = ts.device
        NC = k * H
        NCp = _r8(NC)
        lib, st = _lib.load(), _lib.stream_handle(dev)
        d = _lib.LvFeatDesc(n_win, R, Cin, H, ts.stride(0) if n_win > 1 else L * Cr, 4, 1)
        act = torch.empty(4, n_win, R, H, dtype=torch.float32, device=dev)
        Fh = torch.empty(n_win, R, 64, dtype=torch.bfloat16, device=dev)
        Fl = torch.empty_like(Fh)
        check(lib.vissm_lv_mlp_fwd(ctypes.byref(d), ctypes.byref(_feat_params(ws)), ptr(ts), ptr(act), ptr(Fh),
                                   ptr(Fl), st), "vissm_lv_mlp_fwd")
        Wch = torch.empty(H, NCp, dtype=torch.bfloat16, device=dev)
        Wcl = torch.empty_like(Wch)
        check(lib.vissm_lv_pack(None, None, H, 0, 0, None, None, ptr(conv_w), H, k, NCp, ptr(Wch), ptr(Wcl), st),
              "vissm_lv_pack")
        G = torch.empty(R, NCp, dtype=torch.float32, device=dev)
        C = torch.empty(n_win, Lh, H, dtype=torch.float32, device=dev)
        for w in range(n_win):
            gemm_bf16x3(R, NC, H, Fh[w], Fl[w], 64, False, Wch, Wcl, NCp, True, G, NCp)
            check(lib.vissm_lv_conv_diag(ptr(G), NCp, ptr(conv_b), H, k, s, Lh, ptr(C[w]), st), "vissm_lv_conv_diag")
        ctx.save_for_backward(ts, act, Fh, Fl, Wch, Wcl, *ws)
        ctx.dims = (d, n_win, R, H, k, s, Lh, NC, NCp)
        return C

    @staticmethod
    def backward(ctx, dC):
        ts, act, Fh, Fl, Wch, Wcl, *ws = ctx.saved_tensors
        d, n_win, R, H, k, s, Lh, NC, NCp = ctx.dims
        dev = dC.device
        dC = dC.contiguous()
        lib, st = _lib.load(), _lib.stream_handle(dev)
        dGh = torch.empty(R, NCp, dtype=torch.bfloat16, device=dev)
        dGl = torch.empty_like(dGh)
        dF = torch.empty(n_win, R, H, dtype=torch.float32, device=dev)
        dWc = torch.empty(n_win, H, NC, dtype=torch.float32, device=dev)
        dcb = torch.empty(n_win, H, dtype=torch.float32, device=dev)
        for w in range(n_win):
            check(lib.vissm_lv_conv_diag_bwd(ptr(dC[w]), H, k, s, Lh, R, NCp, ptr(dGh), ptr(dGl), ptr(dcb[w]), st),
                  "vissm_lv_conv_diag_bwd")
            # dF = dG Wc^T (K = k H, split over it: R / 128 row tiles alone would leave the chip empty)
            gemm_bf16x3(R, H, NC, dGh, dGl, NCp, False, Wch, Wcl, NCp, False, dF[w], H, split_k=16)
            # dWc = F^T dG (K = R)
            gemm_bf16x3(H, NC, R, Fh[w], Fl[w], 64, True, dGh, dGl, NCp, True, dWc[w], NC, split_k=8)
        if n_win > 1:
            dWc, dcb = dWc.sum(0, keepdim=True), dcb.sum(0, keepdim=True)
        gr = [torch.empty_like(t) for t in ws[:8]]
        dconv_w = torch.empty_like(ws[8])
        check(lib.vissm_lv_conv_wscatter(ptr(dWc[0]), NC, H, k, H, ptr(dconv_w), st), "vissm_lv_conv_wscatter")
        g = _lib.FeatGrads((ctypes.c_void_p * 4)(ptr(gr[0]), ptr(gr[2]), ptr(gr[4]), ptr(gr[6])),
                           (ctypes.c_void_p * 4)(ptr(gr[1]), ptr(gr[3]), ptr(gr[5]), ptr(gr[7])), None, None)
        nb = lib.vissm_lv_mlp_workspace_size(ctypes.byref(d))
        if nb == 0:
            raise _lib.VissmError(f"vissm_lv_mlp_workspace_size failed: {lib.vissm_last_error().decode()}")
        wsb = _workspace(nb, dev)
        check(lib.vissm_lv_mlp_bwd(ctypes.byref(d), ctypes.byref(_feat_params(ws)), ptr(ts), ptr(act), ptr(dF), H,
                                   ctypes.byref(g), ptr(wsb), nb, st), "vissm_lv_mlp_bwd")
        return (None, None, None, *gr, dconv_w, dcb[0])


def sv_feat_conv(ts, s: int, Lh: int, W0, b0, W1, b1, W2, b2, W3, b3, conv_w, conv_b):
    return SvFeatConvFn.apply(ts, s, Lh, W0, b0, W1, b1, W2, b2, W3, b3, conv_w, conv_b)


class MAFlowFn(torch.autograd.Function):
    """One IAF flow (IAF._create_flow, AR.py:50-85) -> (u_next, logsig)."""

    @staticmethod
    def forward(ctx, shape: FlowShape, win, u, C, theta_term, w_eps, w_hid, b_hid, bn_g, bn_b, w_head, b_head,
                tf=None):
        lib = _lib.load()
        u = _rows(u, shape.L)
        _require_rows(u)
        _require_gpu(C, theta_term, w_eps, w_hid, b_hid, bn_g, bn_b, w_head, b_head, win)
        dev = u.device
        pout = (shape.Lout + 15) // 16 * 16 if shape.pad_out else shape.Lout
        d = shape.desc(_pitch(u, shape.L), pout)
        u_next = _rows_empty(shape.B, shape.Lout, pout, dev)
        logsig = torch.empty(shape.B, dtype=torch.float32, device=dev)
        wsz = lib.vissm_flow_workspace_size(ctypes.byref(d), 0)
        if wsz == 0:
            check(-1, "vissm_flow_workspace_size")
        ws = _workspace(wsz, dev)
        prm = _flow_params(w_eps, w_hid, b_hid, bn_g, bn_b, w_head, b_head, tf)
        check(lib.vissm_flow_fwd(ctypes.byref(d), ctypes.byref(prm), ptr(u), ptr(C), ptr(win), ptr(theta_term),
                                 ptr(u_next), ptr(logsig), ptr(ws), wsz, _lib.stream_handle(dev)),
              "vissm_flow_fwd")
        ctx.shape = shape
        # the theta-fold factors are constants here (theta_term carries their gradient) but are saved like the
        # rest, so autograd's version check catches an in-place change between forward and backward
        tf = tuple(tf) if tf is not None else ()
        ctx.n_tf = len(tf)
        ctx.save_for_backward(win, u, C, theta_term, w_eps, w_hid, b_hid, bn_g, bn_b, w_head, b_head, *tf)
        return u_next, logsig

    @staticmethod
    def backward(ctx, g_next, g_ls):
        lib = _lib.load()
        shape: FlowShape = ctx.shape
        saved = ctx.saved_tensors
        win, u, C, theta_term, w_eps, w_hid, b_hid, bn_g, bn_b, w_head, b_head = saved[:11]
        tf = tuple(saved[11:]) if ctx.n_tf else None
        dev = u.device
        if g_next is None:
            g_next = torch.zeros(shape.B, shape.Lout, dtype=torch.float32, device=dev)
        if g_ls is None:
            g_ls = torch.zeros(shape.B, dtype=torch.float32, device=dev)
        g_next = _rows(g_next, shape.Lout)
        g_ls = g_ls.contiguous()
        if shape.bwd_precision is not None:
            shape = dataclasses.replace(shape, precision=shape.bwd_precision, bwd_precision=None)
        u = _rows(u, shape.L)
        pu = _pitch(u, shape.L)
        d = shape.desc(pu, _pitch(g_next, shape.Lout))
        # the base noise needs no gradient: the bf16 kernels then skip the transposed convolution (the exact-fp32
        # kernels a shape beyond flow5 falls back to always write du)
        need_du = ctx.needs_input_grad[2] or kernel_precision(shape) == _lib.VISSM_PREC_FP32 or _FORCE_DU
        du = _rows_empty(shape.B, shape.L, pu, dev) if need_du else None   # du rows at u's pitch
        dC = torch.empty_like(C)
        dth = torch.empty_like(theta_term)
        gw = [torch.empty_like(t) if t is not None else None for t in (w_eps, w_hid, b_hid, bn_g, bn_b, w_head, b_head)]
        grads = FlowGrads(*[ptr(t) for t in gw])
        wsz = lib.vissm_flow_workspace_size(ctypes.byref(d), 1)
        ws = _workspace(wsz, dev)
        prm = _flow_params(w_eps, w_hid, b_hid, bn_g, bn_b, w_head, b_head, tf)
        check(lib.vissm_flow_bwd(ctypes.byref(d), ctypes.byref(prm), ptr(u), ptr(C), ptr(win), ptr(theta_term),
                                 ptr(g_next), ptr(g_ls), ptr(du), ptr(dC), ptr(dth), ctypes.byref(grads), ptr(ws),
                                 wsz, _lib.stream_handle(dev)), "vissm_flow_bwd")
        return (None, None, du, dC, dth, *gw, None)


def _rows(t: torch.Tensor, n: int) -> torch.Tensor:
    """t as rows of n unit-stride floats at some pitch >= n (VissmFlowDesc.u_pitch / out_pitch); copied only when it
    is not (a transposed or sliced-column view)."""
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < n):
        t = t.contiguous()
    return t


def _pitch(t: torch.Tensor, n: int) -> int:
    return t.stride(0) if t.shape[0] > 1 else n


def _rows_empty(B: int, n: int, pitch: int, device) -> torch.Tensor:
    """[B, n] float32 rows `pitch` floats apart (a column slice of a [B, pitch] buffer)."""
    buf = torch.empty(B, pitch, dtype=torch.float32, device=device)
    return buf if pitch == n else buf[:, :n]


def ma_flow(shape: FlowShape, win, u, C, theta_term, w_eps, w_hid, b_hid, bn_g, bn_b, w_head, b_head, tf=None):
    return MAFlowFn.apply(shape, win, u, C, theta_term, w_eps, w_hid, b_hid, bn_g, bn_b, w_head, b_head, tf)


def ar_fused_supported(shape: FlowShape) -> bool:
    d = shape.desc()
    return bool(_lib.load().vissm_flow_ar_elbo_fused_supported(ctypes.byref(d)))


def ar_last_flow_fused(shape: FlowShape, win, u, C, theta_term, theta, obs, obs_bin, obs_std: float, scale: float,
                       w_eps, w_hid, b_hid, w_head, b_head, tf=None):
    """The last AR(1) flow fused with its ELBO terms (vissm_flow_ar_elbo_fused): one backward-style pass that
    recomputes the flow's output x and differentiates loss = -scale sum_b (sde + obs + logsig) w.r.t. u, C,
    theta_term and the flow's weights (no autograd: the caller routes them; the theta dependence of sde goes
    through vissm_elbo_bwd on x).  Returns (x [B, Lout], logsig [B], du, dC, dtheta_term,
    [g_w_eps, g_w_hid, g_b_hid, g_w_head, g_b_head])."""
    lib = _lib.load()
    u = _rows(u, shape.L)
    _require_rows(u)
    _require_gpu(C, theta_term, theta, obs, obs_bin, w_eps, w_hid, b_hid, w_head, b_head, win)
    dev = u.device
    pu = _pitch(u, shape.L)
    d = shape.desc(pu, 0)
    wsz = lib.vissm_flow_ar_elbo_fused_workspace_size(ctypes.byref(d))
    if wsz == 0:
        raise _lib.VissmError("vissm_flow_ar_elbo_fused: unsupported flow shape")
    ws = _workspace(wsz, dev)
    x = torch.empty(shape.B, shape.Lout, dtype=torch.float32, device=dev)
    logsig = torch.empty(shape.B, dtype=torch.float32, device=dev)
    du = _rows_empty(shape.B, shape.L, pu, dev)
    dC = torch.empty_like(C)
    dth = torch.empty_like(theta_term)
    gw = [torch.empty_like(t) for t in (w_eps, w_hid, b_hid, w_head, b_head)]
    grads = FlowGrads(ptr(gw[0]), ptr(gw[1]), ptr(gw[2]), None, None, ptr(gw[3]), ptr(gw[4]))
    prm = _flow_params(w_eps, w_hid, b_hid, None, None, w_head, b_head, tf)
    check(lib.vissm_flow_ar_elbo_fused(ctypes.byref(d), ctypes.byref(prm), ptr(u), ptr(C), ptr(win), ptr(theta_term),
                                       ptr(theta), ptr(obs), ptr(obs_bin), float(obs_std), float(scale), ptr(x),
                                       ptr(logsig), ptr(du), ptr(dC), ptr(dth), ctypes.byref(grads), ptr(ws), wsz,
                                       _lib.stream_handle(dev)), "vissm_flow_ar_elbo_fused")
    return x, logsig, du, dC, dth, gw


# ---------------------------------------------------------------------------------------
# ELBO log-densities
# ---------------------------------------------------------------------------------------
@dataclass
class ElboFeeds:
    """Per-window observation feeds (device tensors, fp32; win int32 [B] or None)."""
    obs: Optional[torch.Tensor] = None
    obs_bin: Optional[torch.Tensor] = None
    mask: Optional[torch.Tensor] = None
    shift: Optional[torch.Tensor] = None
    dim_one: Optional[torch.Tensor] = None
    win: Optional[torch.Tensor] = None
    n_win: int = 1
    plain_from: Optional[torch.Tensor] = None   # int32 [n_win]: VissmElboData.plain_from (None: NULL)
    obs_list: Optional[torch.Tensor] = None     # int32 [n_win, stride]: VissmElboData.obs_list (None: NULL)

    def cdata(self) -> ElboData:
        ol = self.obs_list
        if ol is not None and (ol.dtype != torch.int32 or ol.dim() != 2 or not ol.is_contiguous()
                               or ol.shape[0] != self.n_win or ol.shape[1] < 1):
            raise ValueError("obs_list must be a contiguous int32 [n_win, stride >= 1] tensor")
        return ElboData(ptr(self.win), ptr(self.obs), ptr(self.obs_bin), ptr(self.mask), ptr(self.shift),
                        ptr(self.dim_one), ptr(self.plain_from), ptr(ol), int(ol.shape[1]) if ol is not None else 0)


class ElboFn(torch.autograd.Function):
    """Path log-densities per sample -> (sde, obs, extra)."""

    @staticmethod
    def forward(ctx, model: int, M: int, dt: float, obs_std: float, feeds: ElboFeeds, z, theta):
        lib = _lib.load()
        _require_gpu(z, theta, feeds.obs, feeds.obs_bin, feeds.mask, feeds.shift, feeds.dim_one, feeds.win)
        B = z.shape[0]
        d = ElboDesc(model, B, M, feeds.n_win, float(dt), float(obs_std))
        data = feeds.cdata()
        sde = torch.empty(B, dtype=torch.float32, device=z.device)
        obs = torch.empty_like(sde)
        extra = torch.empty_like(sde)
        check(lib.vissm_elbo_fwd(ctypes.byref(d), ctypes.byref(data), ptr(z), ptr(theta), ptr(sde), ptr(obs),
                                 ptr(extra), _lib.stream_handle(z.device)), "vissm_elbo_fwd")
        ctx.args = (model, M, dt, obs_std, feeds)
        ctx.save_for_backward(z, theta)
        return sde, obs, extra

    @staticmethod
    def backward(ctx, g_sde, g_obs, g_extra):
        lib = _lib.load()
        model, M, dt, obs_std, feeds = ctx.args
        z, theta = ctx.saved_tensors
        B = z.shape[0]
        zero = None

        def fix(g):
            nonlocal zero
            if g is None:
                if zero is None:
                    zero = torch.zeros(B, dtype=torch.float32, device=z.device)
                return zero
            return g.contiguous()

        g_sde, g_obs, g_extra = fix(g_sde), fix(g_obs), fix(g_extra)
        d = ElboDesc(model, B, M, feeds.n_win, float(dt), float(obs_std))
        data = feeds.cdata()
        dz = torch.empty_like(z)
        dth = torch.empty_like(theta)
        check(lib.vissm_elbo_bwd(ctypes.byref(d), ctypes.byref(data), ptr(z), ptr(theta), ptr(g_sde), ptr(g_obs),
                                 ptr(g_extra), ptr(dz), ptr(dth), _lib.stream_handle(z.device)), "vissm_elbo_bwd")
        return None, None, None, None, None, dz, dth


def elbo_terms(model: int, M: int, dt: float, obs_std: float, feeds: ElboFeeds, z, theta):
    return ElboFn.apply(model, M, dt, obs_std, feeds, z, theta)


def elbo_values_and_theta_grad(model: int, M: int, dt: float, obs_std: float, feeds: ElboFeeds, z, theta,
                               g_sde: torch.Tensor, g_obs: torch.Tensor):
    """(sde, obs) per sample and d(g_sde . sde + g_obs . obs)/d theta for a path z that is a constant (no dz:
    vissm_elbo_bwd with dz = NULL); no autograd."""
    lib = _lib.load()
    _require_gpu(z, theta, g_sde, g_obs, feeds.obs, feeds.obs_bin, feeds.mask, feeds.shift, feeds.dim_one, feeds.win)
    B = z.shape[0]
    d = ElboDesc(model, B, M, feeds.n_win, float(dt), float(obs_std))
    data = feeds.cdata()
    sde = torch.empty(B, dtype=torch.float32, device=z.device)
    obs = torch.empty_like(sde)
    extra = torch.empty_like(sde)
    dth = torch.empty_like(theta)
    st = _lib.stream_handle(z.device)
    if os.environ.get("VISSM_ELBO_TWO_PASS") == "1":   # A/B hook: the two calls, z read twice
        check(lib.vissm_elbo_fwd(ctypes.byref(d), ctypes.byref(data), ptr(z), ptr(theta), ptr(sde), ptr(obs),
                                 ptr(extra), st), "vissm_elbo_fwd")
        check(lib.vissm_elbo_bwd(ctypes.byref(d), ctypes.byref(data), ptr(z), ptr(theta), ptr(g_sde), ptr(g_obs),
                                 None, None, ptr(dth), st), "vissm_elbo_bwd")
        return sde, obs, dth
    # one pass over z for AR(1) (vissm_elbo_fwd then vissm_elbo_bwd with dz = NULL for the other models)
    check(lib.vissm_elbo_fwd_theta_grad(ctypes.byref(d), ctypes.byref(data), ptr(z), ptr(theta), ptr(g_sde),
                                        ptr(g_obs), None, ptr(sde), ptr(obs), ptr(extra), ptr(dth), st),
          "vissm_elbo_fwd_theta_grad")
    return sde, obs, dth


def elbo_values_grad(model: int, M: int, dt: float, obs_std: float, feeds: ElboFeeds, z, theta,
                     g_sde: torch.Tensor, g_obs: Optional[torch.Tensor], g_extra: Optional[torch.Tensor],
                     nwv: Optional[int] = None):
    """(sde, obs, extra) per sample, dz and dtheta of g_sde . sde + g_obs . obs + g_extra . extra in ONE pass over z
    (vissm_elbo_fwd_grad): the training step knows these upstream gradients before the forward.  No autograd: the
    caller feeds dz / dtheta into a multi-root backward (Engine.forward_onepass).  nwv (1, 2 or 4): the LV / SV / FHN
    kernel's waves per trajectory through vissm_elbo_fwd_grad_nwv; None: the library's choice."""
    lib = _lib.load()
    _require_gpu(z, theta, g_sde, feeds.obs, feeds.obs_bin, feeds.mask, feeds.shift, feeds.dim_one, feeds.win,
                 feeds.plain_from, feeds.obs_list)
    B = z.shape[0]
    d = ElboDesc(model, B, M, feeds.n_win, float(dt), float(obs_std))
    data = feeds.cdata()
    sde = torch.empty(B, dtype=torch.float32, device=z.device)
    obs = torch.empty_like(sde)
    extra = torch.empty_like(sde)
    z = z.contiguous()
    dz = torch.empty_like(z)
    dth = torch.empty_like(theta)
    if nwv is not None:
        check(lib.vissm_elbo_fwd_grad_nwv(ctypes.byref(d), ctypes.byref(data), ptr(z), ptr(theta), ptr(g_sde),
                                          ptr(g_obs), ptr(g_extra), ptr(sde), ptr(obs), ptr(extra), ptr(dz), ptr(dth),
                                          int(nwv), _lib.stream_handle(z.device)), "vissm_elbo_fwd_grad_nwv")
        return sde, obs, extra, dz, dth
    check(lib.vissm_elbo_fwd_grad(ctypes.byref(d), ctypes.byref(data), ptr(z), ptr(theta), ptr(g_sde), ptr(g_obs),
                                  ptr(g_extra), ptr(sde), ptr(obs), ptr(extra), ptr(dz), ptr(dth),
                                  _lib.stream_handle(z.device)), "vissm_elbo_fwd_grad")
    return sde, obs, extra, dz, dth


# ---------------------------------------------------------------------------------------
# optimiser
# ---------------------------------------------------------------------------------------
class AdamaxKernel:
    """Fused global-norm clip + Adamax over flat fp32 buffers (optimisers/adamax.py:42-58)."""

    def __init__(self, n: int, device):
        lib = _lib.load()
        self.n = n
        self.wsz = lib.vissm_adamax_workspace_size(n)
        self.ws = _workspace(self.wsz, device)
        self.gnorm = torch.zeros(1, dtype=torch.float32, device=device)
        self.skipped = torch.zeros(1, dtype=torch.int32, device=device)  # guarded steps skipped so far

    def step(self, params, grads, v, m, lr, beta1, beta2, eps=1e-8, clip=0.0, guard=False):
        """guard: skip the update (params and slots untouched, self.skipped += 1) when the global norm
        is not finite, instead of the reference's NaN-everything (vissm_adamax_step_guarded)."""
        lib = _lib.load()
        _require_gpu(params, grads, v, m)
        if guard:
            check(lib.vissm_adamax_step_guarded(ptr(params), ptr(grads), ptr(v), ptr(m), self.n, float(lr),
                                                float(beta1), float(beta2), float(eps), float(clip), ptr(self.gnorm),
                                                ptr(self.skipped), ptr(self.ws), self.wsz,
                                                _lib.stream_handle(params.device)), "vissm_adamax_step_guarded")
        else:
            check(lib.vissm_adamax_step(ptr(params), ptr(grads), ptr(v), ptr(m), self.n, float(lr), float(beta1),
                                        float(beta2), float(eps), float(clip), ptr(self.gnorm), ptr(self.ws), self.wsz,
                                        _lib.stream_handle(params.device)), "vissm_adamax_step")
        return self.gnorm


def sqnorm(x: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    _require_gpu(x)
    n = x.numel()
    wsz = lib.vissm_adamax_workspace_size(n)
    ws = _workspace(wsz, x.device)
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    check(lib.vissm_sqnorm(ptr(x), n, ptr(out), ptr(ws), wsz, _lib.stream_handle(x.device)), "vissm_sqnorm")
    return out


# ---------------------------------------------------------------------------------------
# q(theta) (AR.py:376-391): MAF bijectors over the base draw, one HIP launch each way
# ---------------------------------------------------------------------------------------
def theta_desc(B: int, P: int, n_bij: int, relu: bool, base_loc: float, base_scale: float, perms) -> "_lib.ThetaDesc":
    if not (1 <= P <= _lib.THETA_MAX_P and 1 <= n_bij <= _lib.THETA_MAX_BIJ):
        raise _lib.VissmError(f"q(theta): P={P}, n_bij={n_bij} outside the kernel's range")
    d = _lib.ThetaDesc()
    d.B, d.P, d.n_bij, d.relu = B, P, n_bij, int(bool(relu))
    d.base_loc, d.base_scale = float(base_loc), float(base_scale)
    for i, p in enumerate(perms):
        for q, v in enumerate(p):
            d.perm[i][q] = int(v)
    return d


class ThetaFlowFn(torch.autograd.Function):
    """theta, log q(theta) = q(theta) sample from the base draw x0 (vissm_theta_fwd).  The backward
    (vissm_theta_bwd) adds the MAF variables' gradient straight into `grad_slice` (the flat gradient
    buffer's view of those variables); `anchor` is one of them, an input only so that autograd runs this
    backward (its own gradient is part of grad_slice, so None is returned for it).

    Supported use: loss.backward() into the parameter store (every VI_SSM step and pre-training minimize).
    Under torch.autograd.grad (e.g. optimisers.AdamaxOptimizer.compute_gradients on a loss that reaches theta)
    the q(theta) variables would come back as None while their gradient is still added into the store's flat
    gradient; the model classes never take that route, and INTEGRATION.md states the restriction."""

    @staticmethod
    def forward(ctx, desc_args, w, mask, grad_slice, x0, anchor):
        _require_gpu(w, mask, x0)
        lib = _lib.load()
        B, P = x0.shape
        d = theta_desc(B, P, *desc_args)
        theta = torch.empty(B, P, dtype=torch.float32, device=x0.device)
        logq = torch.empty(B, dtype=torch.float32, device=x0.device)
        check(lib.vissm_theta_fwd(ctypes.byref(d), ptr(w), ptr(mask), ptr(x0), ptr(theta), ptr(logq),
                                  _lib.stream_handle(x0.device)), "vissm_theta_fwd")
        ctx.desc_args, ctx.grad_slice = desc_args, grad_slice
        ctx.save_for_backward(w, mask, x0)
        return theta, logq

    @staticmethod
    def backward(ctx, g_theta, g_logq):
        w, mask, x0 = ctx.saved_tensors
        lib = _lib.load()
        B, P = x0.shape
        d = theta_desc(B, P, *ctx.desc_args)
        g_theta = g_theta.contiguous() if g_theta is not None else None
        g_logq = g_logq.contiguous() if g_logq is not None else None
        ws = _workspace(lib.vissm_theta_workspace_size(ctypes.byref(d)), x0.device)
        check(lib.vissm_theta_bwd(ctypes.byref(d), ptr(w), ptr(mask), ptr(x0), ptr(g_theta), ptr(g_logq),
                                  ptr(ctx.grad_slice), ptr(ws), ws.numel(), _lib.stream_handle(x0.device)),
              "vissm_theta_bwd")
        return None, None, None, None, None, None


# ---------------------------------------------------------------------------------------
# column statistics (posterior summaries)
# ---------------------------------------------------------------------------------------
def _colstat_desc(x: torch.Tensor, n_ranks: int = 1) -> "_lib.ColStatDesc":
    """Descriptor of a [B, n_cols] fp32 GPU matrix with unit inner stride; the rows may lie any pitch >= n_cols
    apart and the view may start anywhere in its storage (x[:, 1:]): the kernels assume 4-byte alignment only."""
    if x.dim() != 2 or not x.is_cuda or x.dtype != torch.float32:
        raise _lib.VissmError("column statistics: a 2-D fp32 GPU tensor is expected (there is deliberately no CPU "
                              "fallback)")
    B, n = x.shape
    if B < 1 or n < 1:
        raise _lib.VissmError(f"column statistics: empty input {tuple(x.shape)}")
    if n > 1 and x.stride(1) != 1:
        raise _lib.VissmError("column statistics: unit inner stride expected")
    pitch = x.stride(0) if B > 1 else n
    if pitch < n:
        raise _lib.VissmError(f"column statistics: row stride {pitch} below the {n} columns")
    return _lib.ColStatDesc(B, n, pitch, n_ranks)


def col_moments(x: torch.Tensor):
    """(sums [2, n_cols] float64: sum and sum of squares over the non-NaN entries of each column, n_valid [n_cols]
    int32) of x [B, n_cols] (vissm_col_moments: fixed-order double accumulation, bitwise reproducible)."""
    lib = _lib.load()
    d = _colstat_desc(x)
    dev = x.device
    sums = torch.empty(2, d.n_cols, dtype=torch.float64, device=dev)
    n_valid = torch.empty(d.n_cols, dtype=torch.int32, device=dev)
    ws = _workspace(lib.vissm_col_moments_workspace_size(ctypes.byref(d)), dev)
    check(lib.vissm_col_moments(ctypes.byref(d), ptr(x), ptr(sums), ptr(n_valid), ptr(ws), _lib.stream_handle(dev)),
          "vissm_col_moments")
    return sums, n_valid


def col_order_stats(x: torch.Tensor, ranks: torch.Tensor, dist=None) -> torch.Tensor:
    """Exact order statistics of the columns of x [B, n_cols]: out[r, c] = the element of 0-based rank ranks[c, r]
    of column c sorted as numpy sorts it (-inf .. +inf, NaN last), [n_ranks, n_cols] fp32.  ranks: int tensor
    [n_cols, n_ranks], or [n_ranks] for every column, at most 16 per column.  Four passes of
    vissm_col_select_hist -> (SUM all-reduce over `dist`, a vi_ssm.DistCtx, when its world > 1: the ranks then index
    the union of all processes' rows) -> vissm_col_select_narrow, then vissm_col_select_decode.  Ranks given on the
    host are checked against [0, rows of all processes); ranks on the device are not read back (no host
    synchronisation here) and the narrowing step clamps them to that range."""
    lib = _lib.load()
    world = dist.world if dist is not None else 1
    if not isinstance(ranks, torch.Tensor) or ranks.dtype not in (torch.int32, torch.int64) or ranks.dim() not in (1, 2):
        raise _lib.VissmError("col_order_stats: ranks must be an int tensor [n_cols, n_ranks] or [n_ranks]")
    n_ranks = ranks.shape[-1]
    if not 1 <= n_ranks <= _lib.COLSTAT_MAX_RANKS:
        raise _lib.VissmError(f"col_order_stats: {n_ranks} ranks per column (1..{_lib.COLSTAT_MAX_RANKS})")
    d = _colstat_desc(x, n_ranks)
    total = d.B * world
    if total >= 2 ** 31:
        raise _lib.VissmError(f"col_order_stats: {total} rows over all processes (must stay below 2^31)")
    if ranks.dim() == 2 and ranks.shape[0] != d.n_cols:
        raise _lib.VissmError(f"col_order_stats: ranks {tuple(ranks.shape)} for {d.n_cols} columns")
    if not ranks.is_cuda and ranks.numel() and (int(ranks.min()) < 0 or int(ranks.max()) >= total):
        raise _lib.VissmError(f"col_order_stats: ranks outside [0, {total})")
    dev = x.device
    rank_left = ranks.to(device=dev, dtype=torch.int32).expand(d.n_cols, n_ranks).contiguous()
    if rank_left.data_ptr() == ranks.data_ptr():
        rank_left = rank_left.clone()   # narrowed in place
    prefix = torch.empty(d.n_cols, n_ranks, dtype=torch.int32, device=dev)   # uint32 keys
    hist = torch.empty(d.n_cols, n_ranks, 256, dtype=torch.int32, device=dev)
    ws = _workspace(lib.vissm_col_select_workspace_size(ctypes.byref(d)), dev)
    st = _lib.stream_handle(dev)
    for p in range(4):
        check(lib.vissm_col_select_hist(ctypes.byref(d), ptr(x), ptr(prefix), p, ptr(hist), ptr(ws), st),
              "vissm_col_select_hist")
        if world > 1:
            dist.all_reduce_(hist)
        check(lib.vissm_col_select_narrow(ctypes.byref(d), ptr(hist), ptr(rank_left), ptr(prefix), p, st),
              "vissm_col_select_narrow")
    out = torch.empty(n_ranks, d.n_cols, dtype=torch.float32, device=dev)
    check(lib.vissm_col_select_decode(ctypes.byref(d), ptr(prefix), ptr(out), st), "vissm_col_select_decode")
    return out


# argument checks shared by sde_simulate, particle_filter and particle_smooth (fn: the caller's name, for the message)
def _sv_refused(fn: str, lacks: str) -> "_lib.VissmError":
    return _lib.VissmError(f"{fn}: no {lacks} for SV (its first coordinate is the observed series)")


def _model_dims(fn: str, model_id: int, sv_lacks: Optional[str] = None):
    """(S, P) of the model; with sv_lacks (what SV does not have) SV is refused."""
    if model_id not in _lib.MODEL_S:
        raise _lib.VissmError(f"{fn}: unknown model {model_id}")
    if sv_lacks is not None and model_id == _lib.MODEL_SV:
        raise _sv_refused(fn, sv_lacks)
    return _lib.MODEL_S[model_id], _lib.MODEL_P[model_id]


def _key_and_row(fn: str, seed: int, row0: int, exc=_lib.VissmError):
    """The Philox key (seed, masked to 64 bits) and first row of a launch as the C ABI takes them."""
    if not 0 <= int(row0) < 2 ** 64:
        raise exc(f"{fn}: row0={row0} outside [0, 2^64)")
    return ctypes.c_uint64(seed & (2 ** 64 - 1)), ctypes.c_uint64(int(row0))


# The checks the particle wrappers share.  The filters and smoothers refuse with VissmError, the chains and the sorted
# filter with ValueError, so each takes the caller's name and its exception class.
def _check_particles(fn: str, exc, N) -> int:
    N = int(N)
    if N not in _lib.PF_PARTICLES:
        raise exc(f"{fn}: N={N} particles, one of {_lib.PF_PARTICLES} expected")
    return N


def _check_positive(fn: str, exc, value, wanted: str):
    """value (dt, obs_std) positive and finite; wanted: the message up to the value."""
    if not 0.0 < float(value) < float("inf"):
        raise exc(f"{fn}: {wanted}, got {value}")


def _check_rows(fn: str, exc, K: int, N: int):
    if K * N >= 2 ** 31:
        raise exc(f"{fn}: K N = {K} * {N} reaches 2^31")


def _check_layout(fn: str, exc, name: str, t: torch.Tensor, shape: tuple, dtype, dev=None):
    """t (loglik_in, ll_cur, x_next, aux_sel): a contiguous GPU tensor of that shape and dtype, on dev where given."""
    if not t.is_cuda or (dev is not None and t.device != dev) or t.dtype != dtype or tuple(t.shape) != shape or \
            not t.is_contiguous():
        kind = {torch.float64: "float64", torch.float32: "fp32", torch.int32: "int32"}[dtype]
        raise exc(f"{fn}: {name}: a contiguous {kind} GPU tensor [{', '.join(map(str, shape))}] expected")


# ---------------------------------------------------------------------------------------
# forward simulation (posterior-predictive forecasts)
# ---------------------------------------------------------------------------------------
def sde_simulate(model_id: int, theta: torch.Tensor, x_start: torch.Tensor, H: int, dt: float, seed: int, row0: int,
                 t0: int = 0, obs_std: Optional[float] = None):
    """Euler-Maruyama paths of one of the four SDEs from per-sample theta [B, P] (raw, as the ELBO takes it) and
    start states x_start [B, S] (vissm_sde_simulate: one lane per sample, the normals drawn in the kernel).  Returns
    (x [B, S, H], y [B, S, H] or None, x_end [B, S]); y = x + obs_std * noise when obs_std is given (not SV).  Sample
    b at step t0 + t consumes entries (t0 + t) NS .. + NS - 1 of the row row0 + b of normal_base(seed, ...) with
    NS = S (2 S with observations), so a call with t0 > 0 and x_start = an earlier call's x_end continues that
    simulation bitwise.  A dead sample (state not finite; LV: outside the positive orthant) is NaN from its dying
    step on.  H = 0: empty x / y and x_end = x_start, no launch."""
    S, P = _model_dims("sde_simulate", model_id)
    _require_gpu(theta, x_start)
    if theta.dtype != torch.float32 or x_start.dtype != torch.float32:
        raise _lib.VissmError("sde_simulate: fp32 theta and x_start expected")
    if theta.dim() != 2 or theta.shape[1] != P or x_start.dim() != 2 or tuple(x_start.shape) != (theta.shape[0], S):
        raise _lib.VissmError(f"sde_simulate: theta [B, {P}] and x_start [B, {S}] expected, got "
                              f"{tuple(theta.shape)} and {tuple(x_start.shape)}")
    with_obs = obs_std is not None
    if with_obs and model_id == _lib.MODEL_SV:
        raise _sv_refused("sde_simulate", "observation model")
    B, H, t0 = theta.shape[0], int(H), int(t0)
    NS = 2 * S if with_obs else S
    if H < 0 or t0 < 0 or (t0 + H) * NS >= 2 ** 31:
        raise _lib.VissmError(f"sde_simulate: bad horizon H={H} t0={t0} ((t0 + H) * {NS} must stay below 2^31)")
    key, row = _key_and_row("sde_simulate", seed, row0)
    dev = theta.device
    x = torch.empty(B, S, H, dtype=torch.float32, device=dev)
    y = torch.empty(B, S, H, dtype=torch.float32, device=dev) if with_obs else None
    if H == 0 or B == 0:
        return x, y, x_start.clone()
    x_end = torch.empty(B, S, dtype=torch.float32, device=dev)
    d = _lib.SimDesc(model_id, B, H, t0, NS, float(dt), float(obs_std) if with_obs else 0.0, int(with_obs))
    check(_lib.load().vissm_sde_simulate(ctypes.byref(d), key, row, ptr(theta), ptr(x_start), ptr(x), ptr(y),
                                         ptr(x_end), _lib.stream_handle(dev)), "vissm_sde_simulate")
    return x, y, x_end


# ---------------------------------------------------------------------------------------
# particle filter, bootstrap or fully adapted proposal (log-evidence and filtering bands)
# ---------------------------------------------------------------------------------------
PF_PROPOSALS = ("bootstrap", "adapted")


@dataclass
class ParticleFilterResult:
    loglik: torch.Tensor                 # [K] float64: loglik_in + the increments (-inf: a dead filter)
    ll_inc: torch.Tensor                 # [K, H] fp32, 0 at unobserved steps
    ess: torch.Tensor                    # [K, H] fp32, N at unobserved steps
    state_end: torch.Tensor              # [K N, S]
    cloud: Optional[torch.Tensor]        # [K N, S, H] post-resampling particles, or None
    #                                      (adapted: post-propagation; may hold NaN particles at observed LV steps)
    q_trace: Optional[torch.Tensor]      # [K, H, N] int64 (the kernel's uint64 weights, below 2^41), or None
    anc_trace: Optional[torch.Tensor]    # [K, H, N] int32, or None


def particle_filter(model_id: int, theta: torch.Tensor, x_start: torch.Tensor, obs: torch.Tensor,
                    obs_bin: torch.Tensor, dt: float, obs_std: float, N: int, seed: int, row0: int, t0: int = 0,
                    loglik_in: Optional[torch.Tensor] = None, cloud: bool = True, trace: bool = False,
                    H: Optional[int] = None, proposal: str = "bootstrap") -> ParticleFilterResult:
    """K bootstrap particle filters of N particles each, one per row of theta [K, P] (raw, as the ELBO takes it), over
    steps t0 .. t0 + H - 1 of obs / obs_bin [S, T_total] (H = T_total - t0 by default); vissm_particle_filter: one
    block per filter, one particle per lane, integer systematic resampling.  x_start: [K N, S], or [S] for every
    particle.  Observation t scores the state after transition t.  Particle (k, i) consumes the normals
    sde_simulate gives row row0 + k N + i under the same seed, so with obs_bin = 0 the cloud is that call's x.  A
    call with t0 > 0, x_start = the previous call's state_end and loglik_in = its loglik continues bitwise.  AR, LV
    and FHN; SV has no observation model and is refused.

    proposal = "adapted" runs the fully adapted auxiliary filter instead (vissm_particle_filter_adapted): at an
    observed step a particle is weighted on the predictive p(y_t | x_t-1) before it moves, and after the resampling
    drawn from p(x_t | x_t-1, y_t) with its own normals.  Same rows, streams, outputs and chaining; a much lower
    variance of loglik where obs_std is small against the process noise.  obs_std > 0 and finite."""
    fn = "particle_filter"
    if proposal not in PF_PROPOSALS:
        raise _lib.VissmError(f"{fn}: proposal {proposal!r}, one of {PF_PROPOSALS} expected")
    if proposal == "adapted":
        _check_positive(fn, _lib.VissmError, obs_std, "the adapted proposal needs a positive, finite obs_std")
    S, _ = _model_dims(fn, model_id, sv_lacks="observation model")

    def x_start_of(n, dev):
        x = x_start.unsqueeze(0).expand(n, S).contiguous() if x_start.dim() == 1 and x_start.shape[0] == S else x_start
        if x.dim() != 2 or tuple(x.shape) != (n, S):
            raise _lib.VissmError(f"{fn}: x_start [{n}, {S}] or [{S}] expected, got {tuple(x.shape)}")
        return x

    def series_of(dev):
        if obs.dim() != 2 or obs.shape[0] != S or obs_bin.shape != obs.shape:
            raise _lib.VissmError(f"{fn}: obs and obs_bin [{S}, T] expected, got {tuple(obs.shape)} and "
                                  f"{tuple(obs_bin.shape)}")
        if any(t.device != dev for t in (x_start, obs, obs_bin)):
            raise _lib.VissmError(f"{fn}: all tensors on one device expected")
        T_total = obs.shape[1]
        return (obs, obs_bin), T_total, f"{T_total} observations ((t0 + H) * {S} must stay below 2^31)"

    entry = "vissm_particle_filter_adapted" if proposal == "adapted" else "vissm_particle_filter"
    return _filter(fn, entry, model_id, S, theta, x_start, (("obs", obs), ("obs_bin", obs_bin)), x_start_of, series_of,
                   dt, False, obs_std, N, seed, row0, t0, loglik_in, cloud, trace, H)


def _filter(fn: str, entry: str, model_id: int, S: int, theta, x_start, up_front: tuple, x_start_of, series_of, dt,
            need_dt: bool, obs_std: float, N, seed, row0, t0, loglik_in, cloud: bool, trace: bool,
            H) -> ParticleFilterResult:
    """particle_filter and sv_filter: fn is the function's name, entry its C entry, S the coordinates of the filtered
    state.  What differs comes from the caller: up_front, the (name, tensor) pairs checked with theta and x_start
    before any shape; x_start_of(K N, dev), the x_start the entry takes (broadcast, its shape checked);
    series_of(dev), the checked series as (the tensors the entry takes after x_start, T_total, the horizon refusal's
    words for it); need_dt, whether dt must be positive and finite; obs_std, the descriptor's (0.0 without one)."""
    exc = _lib.VissmError
    N = _check_particles(fn, exc, N)
    if need_dt:
        _check_positive(fn, exc, dt, "dt must be positive and finite")
    checked = (("theta", theta), ("x_start", x_start)) + up_front
    _require_gpu(*(t for _, t in checked))
    for name, t in checked:
        if t.dtype != torch.float32:
            raise exc(f"{fn}: fp32 {name} expected, got {t.dtype}")
    P = _lib.MODEL_P[model_id]
    if theta.dim() != 2 or theta.shape[1] != P:
        raise exc(f"{fn}: theta [K, {P}] expected, got {tuple(theta.shape)}")
    K, dev = theta.shape[0], theta.device
    _check_rows(fn, exc, K, N)
    x_start = x_start_of(K * N, dev)
    series, T_total, series_words = series_of(dev)
    t0 = int(t0)
    H = T_total - t0 if H is None else int(H)
    if H < 0 or t0 < 0 or t0 + H > T_total or (t0 + H) * S >= 2 ** 31:
        raise exc(f"{fn}: bad horizon H={H} t0={t0} for {series_words}")
    key, row = _key_and_row(fn, seed, row0)
    if loglik_in is not None:
        _check_layout(fn, exc, "loglik_in", loglik_in, (K,), torch.float64, dev)
    loglik = torch.empty(K, dtype=torch.float64, device=dev)
    ll_inc = torch.empty(K, H, dtype=torch.float32, device=dev)
    ess = torch.empty(K, H, dtype=torch.float32, device=dev)
    state_end = torch.empty(K * N, S, dtype=torch.float32, device=dev)
    cl = torch.empty(K * N, S, H, dtype=torch.float32, device=dev) if cloud else None
    qt = torch.empty(K, H, N, dtype=torch.int64, device=dev) if trace else None
    at = torch.empty(K, H, N, dtype=torch.int32, device=dev) if trace else None
    res = ParticleFilterResult(loglik, ll_inc, ess, state_end, cl, qt, at)
    if K == 0:
        return res
    d = _lib.PfDesc(model_id, K, N, H, t0, T_total, float(dt), float(obs_std))
    check(getattr(_lib.load(), entry)(ctypes.byref(d), key, row, ptr(theta), ptr(x_start), *map(ptr, series),
                                      ptr(loglik_in), ptr(loglik), ptr(ll_inc), ptr(ess), ptr(state_end), ptr(cl),
                                      ptr(qt), ptr(at), _lib.stream_handle(dev)), entry)
    return res


# ---------------------------------------------------------------------------------------
# particle smoother (backward simulation over the filter's cloud: smoothing bands)
# ---------------------------------------------------------------------------------------
@dataclass
class ParticleSmoothResult:
    paths: torch.Tensor                  # [K M, S, H] backward trajectories (NaN where no particle could be drawn)
    x_first: torch.Tensor                # [K M, S] = paths[:, :, 0]: the x_next of the call over the steps before
    idx: Optional[torch.Tensor]          # [K M, H] int32 the chosen particle of each step (-1 where NaN), or None
    q_trace: Optional[torch.Tensor]      # [K, H, M, N] int64 (the kernel's uint64 weights, at most 2^40), or None


def particle_smooth(model_id: int, theta: torch.Tensor, cloud: torch.Tensor, dt: float, M: int, seed: int, row0: int,
                    t0: int = 0, x_next: Optional[torch.Tensor] = None, idx: bool = False,
                    trace: bool = False) -> ParticleSmoothResult:
    """M backward-simulation trajectories per filter over cloud [K N, S, H], the equally weighted post-resampling
    particles particle_filter wrote for theta [K, P] (raw); vissm_particle_smooth: one wave per block, one trajectory
    per lane, the selection in integers.  Trajectory (k, j) draws its selection words from Philox row
    row0 + k N + j under `seed` at counter (t0 + t, 2, row).  x_next [K M, S] is the target of the last step (None:
    a uniform draw over the live particles there); a call over the steps before with x_next = this call's x_first
    and its own t0 continues bitwise.  AR, LV and FHN; SV has no filter and is refused."""
    S, _ = _model_dims("particle_smooth", model_id, sv_lacks="particle filter")
    return _smooth("particle_smooth", "vissm_particle_smooth", model_id, S, theta, cloud, dt, False,
                   lambda dev, H, t0: ((), True, " (H >= 1 and t0 + H below 2^31)"), M, seed, row0, t0, x_next, idx,
                   trace)


def _smooth(fn: str, entry: str, model_id: int, S: int, theta, cloud, dt, need_dt: bool, series_of, M, seed, row0, t0,
            x_next, idx: bool, trace: bool) -> ParticleSmoothResult:
    """particle_smooth and sv_smooth: fn is the function's name, entry its C entry, S the cloud's coordinates.  The
    caller hands in need_dt, whether dt must be positive and finite, and series_of(dev, H, t0): (the arguments the
    entry takes between cloud and x_next, whether the series reaches as far as these columns need, the horizon
    refusal's words after H and t0)."""
    exc = _lib.VissmError
    _require_gpu(theta, cloud)
    for name, t in (("theta", theta), ("cloud", cloud)):
        if t.dtype != torch.float32:
            raise exc(f"{fn}: fp32 {name} expected, got {t.dtype}")
    P = _lib.MODEL_P[model_id]
    if theta.dim() != 2 or theta.shape[1] != P or theta.shape[0] < 1:
        raise exc(f"{fn}: theta [K >= 1, {P}] expected, got {tuple(theta.shape)}")
    if need_dt:
        _check_positive(fn, exc, dt, "dt must be positive and finite")
    K, M = theta.shape[0], int(M)
    if cloud.dim() != 3 or cloud.shape[1] != S or cloud.shape[0] % K or not cloud.is_contiguous():
        raise exc(f"{fn}: a contiguous cloud [{K} N, {S}, H] expected, got {tuple(cloud.shape)}")
    N, H, t0 = _check_particles(fn, exc, cloud.shape[0] // K), cloud.shape[2], int(t0)
    if not (_lib.PS_MIN_PATHS <= M <= N and M & (M - 1) == 0):
        raise exc(f"{fn}: M={M} trajectories, a power of two in {_lib.PS_MIN_PATHS} .. N = {N} expected")
    if K > 65535:
        raise exc(f"{fn}: K={K} filters, at most 65535 per call")
    dev = theta.device
    if cloud.device != dev:
        raise exc(f"{fn}: all tensors on one device expected")
    series_args, reaches, horizon_words = series_of(dev, H, t0)
    if H < 1 or t0 < 0 or t0 + H >= 2 ** 31 or not reaches:
        raise exc(f"{fn}: bad horizon H={H} t0={t0}{horizon_words}")
    key, row = _key_and_row(fn, seed, row0)
    theta = theta.contiguous()
    if x_next is not None:
        _check_layout(fn, exc, "x_next", x_next, (K * M, S), torch.float32, dev)
    paths = torch.empty(K * M, S, H, dtype=torch.float32, device=dev)
    x_first = torch.empty(K * M, S, dtype=torch.float32, device=dev)
    ix = torch.empty(K * M, H, dtype=torch.int32, device=dev) if idx else None
    qt = torch.empty(K, H, M, N, dtype=torch.int64, device=dev) if trace else None
    d = _lib.PsDesc(model_id, K, N, M, H, t0, float(dt))
    check(getattr(_lib.load(), entry)(ctypes.byref(d), key, row, ptr(theta), ptr(cloud), *series_args, ptr(x_next),
                                      ptr(paths), ptr(x_first), ptr(ix), ptr(qt), _lib.stream_handle(dev)), entry)
    return ParticleSmoothResult(paths, x_first, ix, qt)


# ---------------------------------------------------------------------------------------
# stochastic volatility: particle filter and smoother of the latent log-volatility
# ---------------------------------------------------------------------------------------
def _sv_series(fn: str, obs: torch.Tensor, dev) -> int:
    """T_total of the series y[0 .. T_total] (a contiguous fp32 GPU vector of T_total + 1 values)."""
    _require_gpu(obs)
    if obs.dtype != torch.float32 or obs.dim() != 1 or obs.shape[0] < 1 or obs.device != dev:
        raise _lib.VissmError(f"{fn}: obs: an fp32 vector y[0 .. T] on theta's device expected, got "
                              f"{obs.dtype} {tuple(obs.shape)}")
    return obs.shape[0] - 1


def _sv_x_start(fn: str, exc, x_start: torch.Tensor, n: int, dev, max_dim: Optional[int] = None) -> torch.Tensor:
    """h at the first step for n particles: one value is broadcast, anything else holds n values (in at most max_dim
    dimensions where given) on theta's device."""
    if x_start.numel() == 1:
        x_start = x_start.reshape(1).expand(n).contiguous()
    if x_start.numel() != n or (max_dim is not None and x_start.dim() > max_dim) or x_start.device != dev:
        raise exc(f"{fn}: x_start [{n}] (or one value) on theta's device expected, got {tuple(x_start.shape)}")
    return x_start


def sv_filter(theta: torch.Tensor, x_start: torch.Tensor, obs: torch.Tensor, dt: float, N: int, seed: int, row0: int,
              t0: int = 0, loglik_in: Optional[torch.Tensor] = None, cloud: bool = True, H: Optional[int] = None,
              trace: bool = False) -> ParticleFilterResult:
    """K particle filters of the stochastic-volatility model's latent log-volatility h, N particles each, one per row
    of theta [K, 4] (raw), over steps t0 .. t0 + H - 1 of the observed series obs = y[0 .. T] (T + 1 values; H = T - t0
    by default); vissm_sv_filter.  Step ta weights each particle's h *before* the move on p(y[ta + 1] | y[ta], h),
    resamples in integers and moves the survivors with the prior transition, which is the exact conditional: the
    fully adapted filter.  x_start: h at step t0, [K N], [K N, 1] or one value for every particle.  Cloud column t is
    an equally weighted sample of p(h_{t0+t+1} | y_{0 : t0+t+1}); shapes, traces and chaining as particle_filter
    with S = 1.  Particle (k, i) uses Philox row row0 + k N + i with AR's stream (n_stream = 1)."""
    fn = "sv_filter"

    def series_of(dev):
        T_total = _sv_series(fn, obs, dev)
        return (obs,), T_total, f"a series of {T_total} transitions"

    return _filter(fn, "vissm_sv_filter", _lib.MODEL_SV, 1, theta, x_start, (),
                   lambda n, dev: _sv_x_start(fn, _lib.VissmError, x_start, n, dev, max_dim=2), series_of, dt, True,
                   0.0, N, seed, row0, t0, loglik_in, cloud, trace, H)


def sv_smooth(theta: torch.Tensor, cloud: torch.Tensor, obs: torch.Tensor, dt: float, M: int, seed: int, row0: int,
              t0: int = 0, x_next: Optional[torch.Tensor] = None, idx: bool = False,
              trace: bool = False) -> ParticleSmoothResult:
    """M backward-simulation trajectories of h per filter over cloud [K N, 1, H], the columns t0 .. t0 + H - 1 that
    sv_filter wrote for theta [K, 4] and the series obs = y[0 .. T]; vissm_sv_smooth.  Column c holds h_{t0+c+1}, and
    y[t0 + c + 2] depends on it, so the backward weight of particle i for the next state xt is the transition density
    times p(y[t0 + c + 2] | y[t0 + c + 1], h_i).  Selection words, x_next [K M, 1] / x_first chaining, the terminal
    rule (x_next None: a uniform draw over the live particles of the last column), idx and trace as particle_smooth.
    Every column with a next state needs y[t0 + c + 2]: t0 + H (+ 1 with x_next) <= T."""
    fn = "sv_smooth"

    def series_of(dev, H, t0):
        T_total = _sv_series(fn, obs, dev)
        need = t0 + H + (1 if x_next is not None else 0)
        return (ptr(obs), T_total), need <= T_total, (": every column with a next state reads y[t0 + c + 2], up to "
                                                      f"y[{need}] of y[0 .. {T_total}]")

    return _smooth(fn, "vissm_sv_smooth", _lib.MODEL_SV, 1, theta, cloud, dt, True, series_of, M, seed, row0, t0,
                   x_next, idx, trace)


# ---------------------------------------------------------------------------------------
# particle marginal Metropolis-Hastings (the theta posterior p(theta | y))
# ---------------------------------------------------------------------------------------
@dataclass
class PmmhResult:
    theta_chain: torch.Tensor            # [C, n_iter, P] the chain's state after each decision
    ll_chain: torch.Tensor               # [C, n_iter] float64, its log-evidence estimate
    accept: torch.Tensor                 # [C, n_iter] int32
    theta_end: torch.Tensor              # [C, P]: theta_cur of the call that continues at it0 + n_iter
    ll_end: torch.Tensor                 # [C] float64: its ll_cur
    theta_prop: Optional[torch.Tensor]   # [C, n_iter, P] the proposals, or None
    ll_prop: Optional[torch.Tensor]      # [C, n_iter] float64 their estimates (-inf: a dead filter), or None
    logu: Optional[torch.Tensor]         # [C, n_iter] float64 the logs of the decisions' uniforms, or None


@dataclass
class PmmhAdaptiveResult(PmmhResult):
    chol_end: torch.Tensor = None               # [C, P, P]: chol_in of the call that continues at it0 + n_iter
    xi_trace: Optional[torch.Tensor] = None     # [C, n_iter, 8] the iterations' normals as the device drew them, or None
    alpha_trace: Optional[torch.Tensor] = None  # [C, n_iter] float64 the acceptance probabilities, or None
    eta_trace: Optional[torch.Tensor] = None    # [C, n_iter] float64 the step sizes (0 from adapt_end on), or None
    chol_trace: Optional[torch.Tensor] = None   # [C, n_iter, P, P] the factor after each iteration, or None


def _adaptive_args(what: str, adapt_end, target_accept, gamma) -> tuple:
    """The refusals the adaptive entries add, by host arithmetic: (adapt_end, target_accept, gamma)."""
    adapt_end, target_accept, gamma = int(adapt_end), float(target_accept), float(gamma)
    if not 0 <= adapt_end < 2 ** 31:
        raise ValueError(f"{what}: adapt_end={adapt_end} outside 0 .. 2^31 - 1 (an absolute iteration)")
    if not 0.0 < target_accept < 1.0:
        raise ValueError(f"{what}: target_accept={target_accept} outside (0, 1)")
    if not 0.0 < gamma <= 1.0:
        raise ValueError(f"{what}: gamma={gamma} outside (0, 1]")
    return adapt_end, target_accept, gamma


def _pmmh_chain(what: str, sv: bool, model_id: int, theta_cur, ll_cur, chol, prior, x_start, obs, obs_bin, dt, obs_std,
                N, n_iter, seed, row0, it0, trace: bool, adapt: Optional[tuple] = None, cpm: Optional[tuple] = None):
    """pmmh, sv_pmmh, pmmh_adaptive, sv_pmmh_adaptive and sv_cpmmh: `what` is the function's name (vissm_<what> its C
    entry), sv says whether the series is the stochastic-volatility model's y[0 .. T] (x_start is then h_start [1],
    obs_bin None and obs_std unused), adapt is None (chol is prop_chol [P, P]) or (adapt_end, target_accept, gamma)
    (chol is chol_in [C, P, P]), cpm is None or the correlated chain's (rho, aux_n, aux_r, aux_sel) (with sv and
    adapt).  The refusals of the C entry, by host arithmetic before any GPU call; then the outputs and the launch.
    The correlated chain keeps the places and words of its own refusals: the series behind the GPU check, as
    sv_filter_sorted refuses it (VissmError), with at least one transition; chol_in with the other tensors; the device
    named with each tensor."""
    exc = ValueError
    if not sv:
        if model_id == _lib.MODEL_SV:
            raise exc(f"{what}: no observation model for SV (its first coordinate is the observed series)")
        if model_id not in _lib.MODEL_S:
            raise exc(f"{what}: unknown model {model_id}")
    S, P = _lib.MODEL_S[model_id], _lib.MODEL_P[model_id]
    N, n_iter, it0 = _check_particles(what, exc, N), int(n_iter), int(it0)
    if sv:
        _check_positive(what, exc, dt, "dt must be positive and finite")
    else:
        _check_positive(what, exc, obs_std, "a positive, finite obs_std expected")
    if cpm is not None:
        rho, aux_n, aux_r, aux_sel = float(cpm[0]), *cpm[1:]
        if not 0.0 <= rho < 1.0 or not 0.0 <= float(torch.tensor(rho, dtype=torch.float32)) < 1.0:
            raise exc(f"{what}: rho={rho} outside [0, 1) (as an fp32 value)")
    if theta_cur.dim() != 2 or theta_cur.shape[1] != P or theta_cur.shape[0] < 1:
        raise exc(f"{what}: theta_cur [C >= 1, {P}] expected, got {tuple(theta_cur.shape)}")
    C = theta_cur.shape[0]
    if n_iter < 0 or it0 < 0 or it0 + n_iter >= 2 ** 31:
        raise exc(f"{what}: bad iterations it0={it0} n_iter={n_iter}")
    if adapt is not None:
        adapt = _adaptive_args(what, *adapt)
    if sv:
        if cpm is None:
            if obs.dim() != 1 or obs.shape[0] < 1 or obs.dtype != torch.float32:
                raise exc(f"{what}: obs: an fp32 vector y[0 .. T] expected, got {obs.dtype} {tuple(obs.shape)}")
            T_total = obs.shape[0] - 1
            if T_total >= 2 ** 31 - 1:
                raise exc(f"{what}: T = {T_total} reaches 2^31 - 1")
        series, shaped = [obs], [("h_start", x_start, (1,))]
    else:
        if obs.dim() != 2 or obs.shape[0] != S or obs_bin.shape != obs.shape:
            raise exc(f"{what}: obs and obs_bin [{S}, T] expected, got {tuple(obs.shape)} and {tuple(obs_bin.shape)}")
        T_total = obs.shape[1]
        if T_total * S >= 2 ** 31:
            raise exc(f"{what}: T S = {T_total} * {S} reaches 2^31")
        series = [obs, obs_bin]
        shaped = [("x_start", x_start, (S,)), ("obs", obs, (S, T_total)), ("obs_bin", obs_bin, (S, T_total))]
    key, row = _key_and_row(what, seed, row0, exc)
    if adapt is None:  # (prop_chol takes its turn below)
        shaped = [("prop_chol", chol, (P, P)), ("prior", prior, (P, 2))] + shaped
    elif cpm is None:
        if chol.dtype != torch.float32 or tuple(chol.shape) != (C, P, P):
            raise exc(f"{what}: fp32 chol_in {[C, P, P]} expected, got {chol.dtype} {tuple(chol.shape)}")
        shaped = [("prior", prior, (P, 2))] + shaped
    else:
        shaped = [("chol_in", chol, (C, P, P)), ("prior", prior, (P, 2))] + shaped
    _require_gpu(theta_cur, chol, prior, x_start, *series)
    dev = theta_cur.device
    if cpm is not None:
        T_total = _sv_series(what, obs, dev)
        if T_total < 1 or T_total >= 2 ** 31 - 1:
            raise exc(f"{what}: T = {T_total}: at least one transition, fewer than 2^31 - 1 expected")
    on_dev = " on one device" if cpm is not None else ""
    for name, x, shape in [("theta_cur", theta_cur, (C, P))] + shaped:
        if x.dtype != torch.float32 or tuple(x.shape) != shape or (on_dev and x.device != dev):
            raise exc(f"{what}: fp32 {name} {list(shape)}{on_dev} expected, got {x.dtype} {tuple(x.shape)}")
    _check_layout(what, exc, "ll_cur", ll_cur, (C,), torch.float64, dev if on_dev else None)
    if any(t.device != dev for t in (ll_cur, chol, prior, x_start, *series)):
        raise exc(f"{what}: all tensors on one device expected")
    if cpm is not None:
        _cpm_aux(what, aux_n, aux_r, (C, 2), T_total, N, dev)
        _check_layout(what, exc, "aux_sel", aux_sel, (C,), torch.int32, dev)
        if bool(((aux_sel != 0) & (aux_sel != 1)).any()):
            raise exc(f"{what}: aux_sel holds a value other than 0 and 1")
    f32, f64 = torch.float32, torch.float64
    e = lambda *shape, dtype=f32: torch.empty(*shape, dtype=dtype, device=dev)
    t = lambda *shape, dtype=f32: e(*shape, dtype=dtype) if trace else None
    chain = [e(C, n_iter, P), e(C, n_iter, dtype=f64), e(C, n_iter, dtype=torch.int32), e(C, P), e(C, dtype=f64)]
    traces = [t(C, n_iter, P), t(C, n_iter, dtype=f64), t(C, n_iter, dtype=f64)]
    if adapt is None:
        scalars, out, result = (), chain + traces, PmmhResult(*chain, *traces)
    else:
        chol_end = e(C, P, P)
        more = [t(C, n_iter, 8), t(C, n_iter, dtype=f64), t(C, n_iter, dtype=f64), t(C, n_iter, P, P)]
        scalars, out = adapt, chain + [chol_end] + traces + more
        if cpm is None:
            result = PmmhAdaptiveResult(*chain, *traces, chol_end, *more)
        else:
            scalars += (ctypes.c_float(rho), ptr(aux_n), ptr(aux_r), ptr(aux_sel))
            result = CpmmhResult(*chain, *traces, chol_end, *more, aux_sel)
    d = _lib.PmmhDesc(model_id, C, N, n_iter, it0, T_total, float(dt), float(obs_std))
    entry = "vissm_" + what
    check(getattr(_lib.load(), entry)(ctypes.byref(d), key, row, *map(ptr, (theta_cur, ll_cur, chol, prior, x_start)),
                                      *map(ptr, series), *scalars, *map(ptr, out), _lib.stream_handle(dev)), entry)
    return result


def pmmh(model_id: int, theta_cur: torch.Tensor, ll_cur: torch.Tensor, prop_chol: torch.Tensor, prior: torch.Tensor,
         x_start: torch.Tensor, obs: torch.Tensor, obs_bin: torch.Tensor, dt: float, obs_std: float, N: int,
         n_iter: int, seed: int, row0: int, it0: int = 0, trace: bool = False) -> PmmhResult:
    """n_iter iterations of C particle marginal Metropolis-Hastings chains, one per row of theta_cur [C, P] (raw, as
    the ELBO takes it); vissm_pmmh: one block per chain, the whole chain in one launch.  An iteration proposes
    theta' = theta + L xi with prop_chol = L [P, P] (lower), estimates log p(y | theta') with the fully adapted filter
    of N particles over obs / obs_bin [S, T] from x_start [S], and accepts iff log u < (ll' - ll) + (lp' - lp), lp the
    independent Gaussian log-prior of prior [P, 2] = (mean, sd).  ll_cur [C] float64 is the estimate that goes with
    theta_cur: particle_filter(proposal="adapted", cloud=False).loglik.  Iteration i of chain c uses the Philox rows
    row0 + (i C + c) N .. + N - 1: its filter is particle_filter's for K = C at row0 + i C N, its proposal and uniform
    sit on counter word 1 = 2 of the first of them.  A call with it0' = it0 + n_iter, theta_cur = theta_end and ll_cur =
    ll_end continues bitwise.  trace: also the proposals, their estimates and log u.  AR, LV and FHN."""
    return _pmmh_chain("pmmh", False, model_id, theta_cur, ll_cur, prop_chol, prior, x_start, obs, obs_bin, dt, obs_std,
                       N, n_iter, seed, row0, it0, trace)


def sv_pmmh(theta_cur: torch.Tensor, ll_cur: torch.Tensor, prop_chol: torch.Tensor, prior: torch.Tensor,
            h_start: torch.Tensor, obs: torch.Tensor, dt: float, N: int, n_iter: int, seed: int, row0: int,
            it0: int = 0, trace: bool = False) -> PmmhResult:
    """pmmh for the stochastic-volatility model, which pmmh refuses: n_iter iterations of C chains, one per row of
    theta_cur [C, 4] (raw); vissm_sv_pmmh: one block per chain, the whole chain in one launch.  An iteration proposes
    theta' = theta + L xi with prop_chol = L [4, 4] (lower), estimates log p(y | theta') with sv_filter's filter of N
    particles (exactly fully adapted) over the series obs = y[0 .. T] (T + 1 values), every particle started at
    h_start [1], and accepts iff log u < (ll' - ll) + (lp' - lp), lp the independent Gaussian log-prior of
    prior [4, 2] = (mean, sd).  ll_cur [C] float64 is the estimate that goes with theta_cur:
    sv_filter(cloud=False).loglik.  Iteration i of chain c uses the Philox rows row0 + (i C + c) N .. + N - 1: its
    filter is sv_filter's for K = C at row0 + i C N, its proposal and uniform sit on counter word 1 = 2 of the first of
    them.  A call with it0' = it0 + n_iter, theta_cur = theta_end and ll_cur = ll_end continues bitwise.  trace: also
    the proposals, their estimates and log u."""
    return _pmmh_chain("sv_pmmh", True, _lib.MODEL_SV, theta_cur, ll_cur, prop_chol, prior, h_start, obs, None, dt, 0.0,
                       N, n_iter, seed, row0, it0, trace)


# ---------------------------------------------------------------------------------------
# adaptive particle marginal Metropolis-Hastings (each chain learns its own proposal factor)
# ---------------------------------------------------------------------------------------
def pmmh_adaptive(model_id: int, theta_cur: torch.Tensor, ll_cur: torch.Tensor, chol_in: torch.Tensor,
                  prior: torch.Tensor, x_start: torch.Tensor, obs: torch.Tensor, obs_bin: torch.Tensor, dt: float,
                  obs_std: float, N: int, n_iter: int, seed: int, row0: int, adapt_end: int,
                  target_accept: float = 0.234, gamma: float = 0.5, it0: int = 0,
                  trace: bool = False) -> PmmhAdaptiveResult:
    """pmmh with a proposal factor per chain, chol_in [C, P, P] (lower; the strict upper part is ignored), that each
    chain adapts itself while its absolute iteration is below adapt_end and keeps frozen after (vissm_pmmh_adaptive;
    robust adaptive Metropolis, Vihola 2012): after the decision of iteration i < adapt_end the factor takes a rank-one
    update with d = eta (alpha - target_accept), eta = min(1, P (i + 1)^-gamma), alpha the proposal's acceptance
    probability.  Every other argument and every PmmhResult field is pmmh's; adapt_end = 0 with chol_in = the shared
    factor tiled is pmmh, bit for bit.  chol_end [C, P, P] is the factor after the last iteration: a call with it0' =
    it0 + n_iter, theta_cur = theta_end, ll_cur = ll_end, chol_in = chol_end and the same adapt_end, target_accept and
    gamma continues bitwise.  trace: also pmmh's traces, the normals, alpha, eta and the factor after each
    iteration.  AR, LV and FHN."""
    return _pmmh_chain("pmmh_adaptive", False, model_id, theta_cur, ll_cur, chol_in, prior, x_start, obs, obs_bin, dt,
                       obs_std, N, n_iter, seed, row0, it0, trace, (adapt_end, target_accept, gamma))


def sv_pmmh_adaptive(theta_cur: torch.Tensor, ll_cur: torch.Tensor, chol_in: torch.Tensor, prior: torch.Tensor,
                     h_start: torch.Tensor, obs: torch.Tensor, dt: float, N: int, n_iter: int, seed: int, row0: int,
                     adapt_end: int, target_accept: float = 0.234, gamma: float = 0.5, it0: int = 0,
                     trace: bool = False) -> PmmhAdaptiveResult:
    """pmmh_adaptive for the stochastic-volatility model: sv_pmmh with a proposal factor per chain, chol_in [C, 4, 4],
    adapted while the absolute iteration is below adapt_end and frozen after (vissm_sv_pmmh_adaptive).  Every other
    argument and every PmmhResult field is sv_pmmh's; the adaptation, chol_end, the chaining and the traces are
    pmmh_adaptive's."""
    return _pmmh_chain("sv_pmmh_adaptive", True, _lib.MODEL_SV, theta_cur, ll_cur, chol_in, prior, h_start, obs, None,
                       dt, 0.0, N, n_iter, seed, row0, it0, trace, (adapt_end, target_accept, gamma))


# ---------------------------------------------------------------------------------------
# correlated pseudo-marginal chain of the stochastic-volatility model (sorted filter, carried noise)
# ---------------------------------------------------------------------------------------
@dataclass
class SortedFilterResult:
    loglik: torch.Tensor                    # [K] float64 (-inf: a dead filter)
    ll_inc: torch.Tensor                    # [K, T] fp32 (NaN from the step a filter died at)
    cloud: Optional[torch.Tensor]           # [K, T, N] h after the move, in slot order, or None
    sorted_trace: Optional[torch.Tensor]    # [K, T, N] the pre-step states as sorted, or None
    q_trace: Optional[torch.Tensor]         # [K, T, N] int64 the integer weights of the sorted states, or None
    anc_trace: Optional[torch.Tensor]       # [K, T, N] int32 positions in the sorted array, or None
    u_trace: Optional[torch.Tensor]         # [K, T] int32 the resampling integers (below 2^24), or None


@dataclass
class CpmmhResult(PmmhAdaptiveResult):
    aux_sel: torch.Tensor = None            # [C] int32: the tensor passed in, after the launch


def cpm_groups(T: int) -> int:
    """G = ceil(T / 4): the Philox groups of a row of T move normals."""
    return (int(T) + 3) // 4


def _cpm_aux(fn: str, aux_n, aux_r, lead: tuple, T: int, N: int, dev):
    G = cpm_groups(T)
    for name, t, shape in (("aux_n", aux_n, lead + (G, N, 4)), ("aux_r", aux_r, lead + (T,))):
        if not t.is_cuda or t.device != dev or t.dtype != torch.float32 or tuple(t.shape) != shape or \
                not t.is_contiguous():
            raise ValueError(f"{fn}: {name}: a contiguous fp32 tensor {list(shape)} on theta's device expected, got "
                             f"{t.dtype} {tuple(t.shape)}")


def sv_filter_sorted(theta: torch.Tensor, x_start: torch.Tensor, obs: torch.Tensor, dt: float, N: int,
                     aux_n: torch.Tensor, aux_r: torch.Tensor, cloud: bool = False,
                     trace: bool = False) -> SortedFilterResult:
    """K particle filters of the stochastic-volatility model over the whole series obs = y[0 .. T], all randomness
    given: aux_n [K, G, N, 4] holds the move normals (entry (t, j) at [k, t // 4, j, t % 4], G = ceil(T / 4)) and
    aux_r [K, T] the resampling normals; vissm_sv_filter_sorted.  Each step sorts the pre-step states ascending (dead
    particles last), weighs, resamples with U = floor(Phi(aux_r[t]) 2^24) and moves position j's ancestor with
    aux_n(t, j): sv_filter's filter with a sort before the scan, so that nearby aux give nearby estimates.  x_start:
    [K N] or one value.  cloud: also h after each move [K, T, N]; trace: also the sorted states, the integer weights,
    the ancestors and U.  Nothing is drawn: two calls are bitwise equal."""
    fn, exc = "sv_filter_sorted", ValueError
    N = _check_particles(fn, exc, N)
    _check_positive(fn, exc, dt, "dt must be positive and finite")
    _require_gpu(theta, x_start)
    if theta.dtype != torch.float32 or x_start.dtype != torch.float32 or theta.dim() != 2 or theta.shape[1] != 4:
        raise exc(f"{fn}: fp32 theta [K, 4] and x_start expected, got {tuple(theta.shape)}")
    K, dev = theta.shape[0], theta.device
    _check_rows(fn, exc, K, N)
    x_start = _sv_x_start(fn, exc, x_start, K * N, dev)
    T = _sv_series(fn, obs, dev)
    if T < 1:
        raise exc(f"{fn}: a series of at least one transition expected")
    _cpm_aux(fn, aux_n, aux_r, (K,), T, N, dev)
    e = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device=dev)
    loglik, ll_inc = e(K, dtype=torch.float64), e(K, T)
    cl = e(K, T, N) if cloud else None
    st = e(K, T, N) if trace else None
    qt = e(K, T, N, dtype=torch.int64) if trace else None
    at = e(K, T, N, dtype=torch.int32) if trace else None
    ut = e(K, T, dtype=torch.int32) if trace else None
    res = SortedFilterResult(loglik, ll_inc, cl, st, qt, at, ut)
    if K == 0:
        return res
    d = _lib.PfDesc(_lib.MODEL_SV, K, N, T, 0, T, float(dt), 0.0)
    check(_lib.load().vissm_sv_filter_sorted(ctypes.byref(d), ptr(theta), ptr(x_start), ptr(obs), ptr(aux_n),
                                             ptr(aux_r), ptr(loglik), ptr(ll_inc), ptr(cl), ptr(st), ptr(qt), ptr(at),
                                             ptr(ut), _lib.stream_handle(dev)), "vissm_sv_filter_sorted")
    return res


def cpm_fresh_aux(C: int, T: int, N: int, seed: int, row0: int, device="cuda"):
    """A fresh auxiliary state for sv_cpmmh: (aux_n [C, 2, G, N, 4], aux_r [C, 2, T], aux_sel [C] int32).  Half 0 holds
    independent N(0, 1) values -- the move normal (t, j) of chain c is entry t of row row0 + c N + j of
    normal_base(seed, ...), its resampling normal t entry t of row row0 + C N + c -- half 1 and aux_sel are zero.  The
    ll_cur that goes with it is sv_filter_sorted(theta_cur, h_start, obs, dt, N, aux_n[:, 0], aux_r[:, 0]).loglik."""
    C, T, N = int(C), int(T), int(N)
    if C < 1 or T < 1 or N not in _lib.PF_PARTICLES:
        raise ValueError(f"cpm_fresh_aux: C={C} (>= 1), T={T} (>= 1), N={N} (one of {_lib.PF_PARTICLES}) expected")
    if not 0 <= int(row0) < 2 ** 64 - C * (N + 1):
        raise ValueError(f"cpm_fresh_aux: row0={row0} outside [0, 2^64 - C (N + 1))")
    G = cpm_groups(T)
    dev = torch.device(device)
    eps, _ = normal_base(seed, int(row0), C * N, T, 1, dev)
    aux_n = torch.zeros(C, 2, G, N, 4, dtype=torch.float32, device=dev)
    pad = torch.zeros(C, N, 4 * G, dtype=torch.float32, device=dev)
    pad[:, :, :T] = eps.view(C, N, T)
    aux_n[:, 0] = pad.view(C, N, G, 4).permute(0, 2, 1, 3)
    aux_r = torch.zeros(C, 2, T, dtype=torch.float32, device=dev)
    aux_r[:, 0] = normal_base(seed, int(row0) + C * N, C, T, 1, dev)[0]
    return aux_n, aux_r, torch.zeros(C, dtype=torch.int32, device=dev)


def sv_cpmmh(theta_cur: torch.Tensor, ll_cur: torch.Tensor, chol_in: torch.Tensor, prior: torch.Tensor,
             h_start: torch.Tensor, obs: torch.Tensor, dt: float, N: int, n_iter: int, seed: int, row0: int,
             rho: float, aux_n: torch.Tensor, aux_r: torch.Tensor, aux_sel: torch.Tensor, adapt_end: int = 0,
             target_accept: float = 0.234, gamma: float = 0.5, it0: int = 0, trace: bool = False) -> CpmmhResult:
    """sv_pmmh_adaptive as a correlated pseudo-marginal chain (vissm_sv_cpmmh; Deligiannidis, Doucet & Pitt 2018): the
    chain carries its filter's random numbers, proposes them by u' = rho u + sqrt(1 - rho^2) eps and estimates
    log p(y | theta') with sv_filter_sorted on the proposed numbers, so the noise of ll' - ll is far below the
    independent filter's at the same N.  aux_n [C, 2, G, N, 4], aux_r [C, 2, T] and aux_sel [C] int32 (cpm_fresh_aux)
    are MUTATED IN PLACE: the half aux_sel[c] names belongs to (theta_cur[c], ll_cur[c]) -- ll_cur must be
    sv_filter_sorted's estimate on that half -- the proposal is written to the other half and acceptance flips
    aux_sel[c].  eps are the normals sv_pmmh's filter would consume in the same iteration (rows row0 + (i C + c) N + j).
    adapt_end = 0 is the fixed-proposal chain with the factors chol_in [C, 4, 4].  A call with it0' = it0 + n_iter,
    theta_end, ll_end, chol_end and the same three aux tensors continues bitwise.  Every other argument, the outputs
    and the traces are sv_pmmh_adaptive's; the result also holds aux_sel (the same tensor)."""
    return _pmmh_chain("sv_cpmmh", True, _lib.MODEL_SV, theta_cur, ll_cur, chol_in, prior, h_start, obs, None, dt, 0.0,
                       N, n_iter, seed, row0, it0, trace, (adapt_end, target_accept, gamma),
                       (rho, aux_n, aux_r, aux_sel))
