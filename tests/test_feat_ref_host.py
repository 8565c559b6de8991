"""tests/feat_ref.py (the float64 forms the feature kernels' GPU tests compare against) checked without a GPU:

* the staged LV / SV references, composed in the order LvFeatConvFn / SvFeatConvFn chain the stages, equal the
  whole-branch torch forms of tests/test_gpu_lvfeat.py / test_gpu_svfeat.py in float64 to 1e-12, values and
  gradients; the fused branch's reference equals test_gpu_feat._torch_ref the same way;
* vissm_lv_conv_diag / _bwd and vissm_lv_pack / vissm_lv_conv_wscatter are adjoint pairs, <A x, y> = <x, A^T y>;
* the sequential fp32 diagonal sum is the float64 one to fp32 rounding, and SV's input assembly is the cat form."""
import numpy as np
import pytest
import torch

from tests import feat_ref as R

F64 = torch.float64


def _rand(g, *sh, sc=1.0):
    return torch.randn(*sh, generator=g, dtype=F64) * sc


def _close(a, b, tol=1e-12):
    a, b = a.detach(), b.detach()
    err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
    assert err <= tol, err


def _lv_weights(g, R_, U, k, Cin, H):
    return [_rand(g, Cin, H, sc=0.3), _rand(g, H, sc=0.1), _rand(g, H, H, sc=0.15), _rand(g, H, sc=0.1),
            _rand(g, H, H, sc=0.15), _rand(g, H, sc=0.1), _rand(g, H, U, sc=0.15), _rand(g, U, sc=0.1),
            _rand(g, k, 1 + R_, H, sc=0.02), _rand(g, H, sc=0.1)]


@pytest.mark.parametrize("R_,U,k,s,Cin,H", [(37, 29, 5, 1, 6, 11), (40, 33, 4, 2, 13, 7)])
def test_lv_staged_reference_is_the_torch_form(monkeypatch, R_, U, k, s, Cin, H):
    from tests import test_gpu_lvfeat as T
    from viforssms_amd.linalg import linear
    monkeypatch.setattr(T, "DEV", "cpu")
    g = torch.Generator().manual_seed(R_ + U)
    ws = [w.requires_grad_(True) for w in _lv_weights(g, R_, U, k, Cin, H)]
    h0 = _rand(g, 2, R_, Cin)
    Lh = (U - k) // s + 1
    dC = _rand(g, 2, Lh, H)
    Cs = R.lv_branch_staged(h0, ws, s, Lh)
    gs = torch.autograd.grad(Cs, ws, dC)
    Ct = torch.cat([T._torch_form(h0[w:w + 1], ws, s, Lh, linear) for w in range(2)])   # the form takes one window
    gt = torch.autograd.grad(Ct, ws, dC)
    _close(Cs, Ct)
    for i, (a, b) in enumerate(zip(gs, gt)):
        if i == 8:
            assert float(a[:, 0, :].abs().max()) == 0.0
        _close(a, b)


@pytest.mark.parametrize("L,Cr,k,s,H", [(31, 5, 6, 1, 9), (40, 8, 5, 2, 12)])
def test_sv_staged_reference_is_the_torch_form(monkeypatch, L, Cr, k, s, H):
    from tests import test_gpu_svfeat as T
    monkeypatch.setattr(T, "DEV", "cpu")
    g = torch.Generator().manual_seed(L + k)
    Cin = 2 * Cr - 2
    ws = [_rand(g, Cin, H, sc=0.3), _rand(g, H, sc=0.1), _rand(g, H, H, sc=0.15), _rand(g, H, sc=0.1),
          _rand(g, H, H, sc=0.15), _rand(g, H, sc=0.1), _rand(g, H, H, sc=0.15), _rand(g, H, sc=0.1),
          _rand(g, k, 1 + H, H, sc=0.03), _rand(g, H, sc=0.1)]
    ws = [w.requires_grad_(True) for w in ws]
    ts = _rand(g, 2, L, Cr)
    Lh = (L - 1 - k) // s + 1
    dC = _rand(g, 2, Lh, H)
    Cs = R.sv_branch_staged(ts, ws, s, Lh)
    gs = torch.autograd.grad(Cs, ws, dC)
    Ct = T._torch_form(ts, ws, s, Lh)
    gt = torch.autograd.grad(Ct, ws, dC)
    _close(Cs, Ct)
    for a, b in zip(gs, gt):
        _close(a, b)
    # the input assembly alone: the loop form against the reference's concatenation
    cat = torch.cat([ts[:, 1:, :], ts[:, 1:, :-2] - ts[:, :-1, :-2]], 2)
    assert torch.equal(R.sv_input(ts), cat)


@pytest.mark.parametrize("n_win,Lf,Cin,H,k,s", [(2, 23, 3, 7, 5, 1), (1, 30, 6, 9, 4, 2), (3, 9, 3, 7, 9, 1)])
def test_feat_reference_is_the_torch_form(monkeypatch, n_win, Lf, Cin, H, k, s):
    from tests import test_gpu_feat as T
    g = torch.Generator().manual_seed(Lf + k)
    Lh = (Lf - k) // s + 1
    ws = [_rand(g, Cin, H, sc=Cin ** -0.5), _rand(g, H, sc=0.1)]
    for _ in range(3):
        ws += [_rand(g, H, H, sc=H ** -0.5), _rand(g, H, sc=0.1)]
    ws += [_rand(g, k, 1 + H, H, sc=(k * H) ** -0.5), _rand(g, H, sc=0.1)]
    h0, dC = _rand(g, n_win, Lf, Cin), _rand(g, n_win, Lh, H)
    C, acts, gr = R.feat_conv_grads(h0, ws, s, Lh, dC)
    wt = [w.clone().requires_grad_(True) for w in ws]
    Ct = T._torch_ref(h0, s, Lh, wt)
    gt = torch.autograd.grad(Ct, wt, dC)
    _close(C, Ct.detach())
    assert len(acts) == 4 and acts[3].shape == (n_win, Lf, H)
    for i, (a, b) in enumerate(zip(gr, gt)):
        if i == 8:
            assert float(a[:, 0, :].abs().max()) == 0.0
        _close(a, b)


@pytest.mark.parametrize("H,k,s,Lh,extra_u,extra_ld", [(7, 5, 1, 9, 0, 0), (5, 4, 2, 6, 3, 2), (3, 1, 2, 4, 1, 5)])
def test_diag_pair_is_adjoint(H, k, s, Lh, extra_u, extra_ld):
    g = torch.Generator().manual_seed(H * k + Lh)
    U, ldg = s * (Lh - 1) + k + extra_u, k * H + extra_ld
    G, y = _rand(g, U, ldg), _rand(g, Lh, H)
    Ax = R.diag(G, torch.zeros(H, dtype=F64), H, k, s, Lh)
    Aty, db = R.diag_bwd(y, H, k, s, Lh, U, ldg)
    lhs, rhs = float((Ax * y).sum()), float((G * Aty).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)
    # the bias: d/db of <diag(G, b), y> is the column sum
    _close(db, y.sum(0))
    # zeros of the transpose: off the taps' diagonals, past k H, rows past the last tap
    assert float(Aty[:, k * H:].abs().sum()) == 0.0 and float(Aty[s * (Lh - 1) + k:].abs().sum()) == 0.0
    assert int((Aty != 0).sum()) == Lh * k * H


@pytest.mark.parametrize("R_,k,H,extra_ld", [(6, 3, 5, 0), (9, 4, 7, 3)])
def test_pack_scatter_pair_is_adjoint(R_, k, H, extra_ld):
    g = torch.Generator().manual_seed(R_ + k)
    ldc = k * H + extra_ld
    cw, Y = _rand(g, k, 1 + R_, H), _rand(g, R_, ldc)
    lhs = float((R.pack_wc(cw, R_, k, H, ldc) * Y).sum())
    At = R.wscatter(Y, R_, k, H)
    rhs = float((cw * At).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)
    assert float(At[:, 0, :].abs().max()) == 0.0
    assert float(R.pack_wc(cw, R_, k, H, ldc)[:, k * H:].abs().sum()) == 0.0


def test_pack_w3b_layout():
    g = torch.Generator().manual_seed(3)
    H, U, ldw = 5, 11, 16
    w3, b3 = _rand(g, H, U), _rand(g, U)
    W = R.pack_w3b(w3, b3, H, U, ldw)
    assert W.shape == (64, ldw)
    assert torch.equal(W[:H, :U], w3) and torch.equal(W[H, :U], b3)
    assert float(W[H + 1:].abs().sum()) == 0.0 and float(W[:, U:].abs().sum()) == 0.0
    # [H3 | 1 | 0] W3b is the layer with its bias
    H3 = _rand(g, 4, H)
    H3b = torch.zeros(4, 64, dtype=F64)
    H3b[:, :H], H3b[:, H] = H3, 1
    _close((H3b @ W)[:, :U], H3 @ w3 + b3)


def test_sequential_fp32_diag_is_the_float64_sum_to_rounding():
    g = torch.Generator().manual_seed(4)
    H, k, s, Lh = 6, 9, 2, 13
    G = torch.randn(s * (Lh - 1) + k + 2, k * H + 3, generator=g)
    cb = torch.randn(H, generator=g)
    seq = R.diag_f32_sequential(G.numpy(), cb.numpy(), H, k, s, Lh)
    assert seq.dtype == np.float32
    ref = R.diag(G.double(), cb.double(), H, k, s, Lh).numpy()
    mag = R.diag(G.double().abs(), cb.double().abs(), H, k, s, Lh).numpy()
    assert np.all(np.abs(seq - ref) <= (k + 1) * 2.0 ** -24 * mag)


def test_split_bf16_planes():
    x = torch.randn(1000, generator=torch.Generator().manual_seed(5))
    hi, lo = R.split_bf16(x)
    assert hi.dtype == lo.dtype == torch.bfloat16
    assert float((hi.float() + lo.float() - x).abs().max()) <= 2.0 ** -16 * float(x.abs().max())
