"""Plain float64 forms of the window-shared feature branch and of every stage of the LV / SV branch, on the CPU.

Written from the operations' definitions in include/vissm.h (and the reference layers they replace: AR.py:53-62,
lotka_volterra_partial.py:71-82, SV_dense.py:50-62), one loop or one matmul per definition: nothing here knows
the kernels' tiling, their launch order or viforssms_amd/ops.py.  tests/test_feat_ref_host.py holds these forms
against the whole-branch torch forms of the GPU tests (no GPU needed); the GPU tests hold the kernels against
these.

Weights come as the list ws = [W0, b0, W1, b1, W2, b2, W3, b3, conv_w, conv_b] of float64 CPU tensors."""
import numpy as np
import torch

F64 = torch.float64


def to64(t):
    return t.detach().to("cpu", F64)


def elu(x):
    return torch.where(x > 0, x, torch.expm1(x))


def elu_d_out(y):
    """elu'(x) from the output y = elu(x)"""
    return torch.where(y > 0, torch.ones_like(y), y + 1)


# ---------------------------------------------------------------------------------------
# vissm_feat_fwd / vissm_feat_bwd
# ---------------------------------------------------------------------------------------
def mlp(h, ws, n_layers):
    """the dense + ELU layers: every layer's output, [n_layers] tensors [.., rows, H]"""
    acts = []
    for l in range(n_layers):
        h = elu(h @ ws[2 * l] + ws[2 * l + 1])
        acts.append(h)
    return acts


def feat_conv(h0, ws, s, Lh):
    """C [n_win][Lh][H] = conv_b + sum_j F[s m + j] conv_w[j][1:], F the fourth layer's output; and the four layers'
    outputs.  h0 [n_win][Lf][Cin]."""
    acts = mlp(h0, ws, 4)
    F, cw, cb = acts[3], ws[8], ws[9]
    k, H = cw.shape[0], cw.shape[2]
    C = cb.expand(h0.shape[0], Lh, H).clone()
    for m in range(Lh):
        # [n_win][k][H] x [k][H][H]: all taps of one output position
        C[:, m, :] = cb + torch.einsum("wji,jio->wo", F[:, s * m:s * m + k, :], cw[:, 1:, :])
    return C, acts


def feat_conv_grads(h0, ws, s, Lh, dC):
    """(C, acts, grads of ws) by autograd; the conv kernel's sample channel 0 gets a zero gradient"""
    wd = [to64(w).requires_grad_(True) for w in ws]
    C, acts = feat_conv(to64(h0), wd, s, Lh)
    g = torch.autograd.grad(C, wd, to64(dC))
    return C.detach(), [a.detach() for a in acts], list(g)


# ---------------------------------------------------------------------------------------
# vissm_lv_mlp_fwd / _bwd
# ---------------------------------------------------------------------------------------
def sv_input(ts):
    """SV's MLP input from the window's time features ts [n_win][L][Cr] (include/vissm.h, VissmLvFeatDesc): row r is
    [ts[r + 1][0 .. Cr), ts[r + 1][c] - ts[r][c] for c < Cr - 2]: [n_win][L - 1][2 Cr - 2]"""
    n_win, L, Cr = ts.shape
    out = torch.empty(n_win, L - 1, 2 * Cr - 2, dtype=ts.dtype)
    for r in range(L - 1):
        out[:, r, :Cr] = ts[:, r + 1, :]
        for c in range(Cr - 2):
            out[:, r, Cr + c] = ts[:, r + 1, c] - ts[:, r, c]
    return out


def lv_mlp(h0, ws, n_layers, sv_diff):
    x = sv_input(h0) if sv_diff else h0
    return mlp(x, ws, n_layers)


def lv_mlp_grads(h0, ws, n_layers, sv_diff, dH):
    """(acts, grads of ws[:2 n_layers]) for the gradient dH [n_win][R][H] of the last layer's output"""
    wd = [to64(w).requires_grad_(True) for w in ws[:2 * n_layers]]
    acts = lv_mlp(to64(h0), wd, n_layers, sv_diff)
    g = torch.autograd.grad(acts[-1], wd, to64(dH))
    return [a.detach() for a in acts], list(g)


# ---------------------------------------------------------------------------------------
# bf16 planes
# ---------------------------------------------------------------------------------------
def split_bf16(x32):
    """hi = bf16(x), lo = bf16(x - hi), round to nearest even, of an fp32 tensor"""
    hi = x32.to(torch.bfloat16)
    return hi, (x32 - hi.float()).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------
# vissm_lv_pack / vissm_lv_conv_wscatter
# ---------------------------------------------------------------------------------------
def pack_w3b(w3, b3, H, U, ldw):
    """W3b [64][ldw]: rows < H the kernel w3 [H][U], row H its bias, zeros elsewhere"""
    out = torch.zeros(64, ldw, dtype=w3.dtype)
    out[:H, :U] = w3
    out[H, :U] = b3
    return out


def pack_wc(conv_w, R, k, H, ldc):
    """Wc [R][ldc]: Wc[r][j H + h] = conv_w[j][1 + r][h], zeros past k H"""
    out = torch.zeros(R, ldc, dtype=conv_w.dtype)
    for j in range(k):
        for r in range(R):
            out[r, j * H:(j + 1) * H] = conv_w[j, 1 + r, :]
    return out


def wscatter(dWc, R, k, H):
    """dconv_w [k][1 + R][H]: dconv_w[j][1 + r][h] = dWc[r][j H + h], channel 0 zero (the transpose of pack_wc)"""
    out = torch.zeros(k, 1 + R, H, dtype=dWc.dtype)
    for j in range(k):
        for r in range(R):
            out[j, 1 + r, :] = dWc[r, j * H:(j + 1) * H]
    return out


# ---------------------------------------------------------------------------------------
# vissm_lv_conv_diag / _bwd
# ---------------------------------------------------------------------------------------
def diag(G, conv_b, H, k, s, Lh):
    """C[m][h] = conv_b[h] + sum_j G[s m + j][j H + h]"""
    C = torch.zeros(Lh, H, dtype=G.dtype)
    for m in range(Lh):
        for j in range(k):
            C[m] += G[s * m + j, j * H:(j + 1) * H]
    return C + conv_b


def diag_f32_sequential(G, conv_b, H, k, s, Lh):
    """the same sum in fp32, started at conv_b[h], j ascending (numpy: one rounding per add)"""
    G = np.asarray(G, dtype=np.float32)
    C = np.repeat(np.asarray(conv_b, dtype=np.float32)[None, :], Lh, 0).copy()
    for j in range(k):
        C = (C + G[j:j + s * (Lh - 1) + 1:s, j * H:(j + 1) * H]).astype(np.float32)
    return C


def diag_bwd(dC, H, k, s, Lh, U, ldg):
    """the transpose of diag's sum: dG [U][ldg], dG[s m + j][j H + h] = dC[m][h], zeros elsewhere; and
    dconv_b[h] = sum_m dC[m][h]"""
    dG = torch.zeros(U, ldg, dtype=dC.dtype)
    for m in range(Lh):
        for j in range(k):
            dG[s * m + j, j * H:(j + 1) * H] = dC[m]
    return dG, dC.sum(0)


# ---------------------------------------------------------------------------------------
# the stages in the order the LV / SV branches chain them (float64 throughout: no bf16 rounding)
# ---------------------------------------------------------------------------------------
def lv_branch_staged(h0, ws, s, Lh):
    """LV: three layers, the time-mixing layer as [H3 | 1] W3b, G = D^T Wc, the diagonal sum; per window"""
    n_win, R, _ = h0.shape
    H, U, k = ws[0].shape[1], ws[6].shape[1], ws[8].shape[0]
    W3b = pack_w3b(ws[6], ws[7], H, U, U)
    Wc = pack_wc(ws[8], R, k, H, k * H)
    out = []
    for w in range(n_win):
        H3 = lv_mlp(h0[w:w + 1], ws, 3, False)[-1][0]
        H3b = torch.zeros(R, 64, dtype=h0.dtype)
        H3b[:, :H] = H3
        H3b[:, H] = 1
        D = elu(H3b @ W3b)                      # [R][U]
        G = D.t() @ Wc                          # [U][k H]
        out.append(diag(G, ws[9], H, k, s, Lh))
    return torch.stack(out)


def sv_branch_staged(ts, ws, s, Lh):
    """SV: four layers over the differenced input, G = F Wc, the diagonal sum; per window"""
    n_win = ts.shape[0]
    H, k = ws[0].shape[1], ws[8].shape[0]
    Wc = pack_wc(ws[8], H, k, H, k * H)
    out = []
    for w in range(n_win):
        F = lv_mlp(ts[w:w + 1], ws, 4, True)[-1][0]
        out.append(diag(F @ Wc, ws[9], H, k, s, Lh))
    return torch.stack(out)


# ---------------------------------------------------------------------------------------
# error measures of the kernels' tests
# ---------------------------------------------------------------------------------------
def rel_l2(a, ref):
    a, ref = to64(a), to64(ref)
    return float((a - ref).norm() / ref.norm().clamp_min(1e-30))


def max_rel_scale(a, ref):
    """largest |a - ref| over the tensor's largest |ref|"""
    a, ref = to64(a), to64(ref)
    return float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300))
