"""An independent float64 reference of ONE IAF flow at the C ABI (vissm_flow_fwd / vissm_flow_bwd /
vissm_flow_ar_elbo_fused), restated from the formula block of include/vissm.h ("One IAF flow of the neural-MA
sampler"), not from oracle.nma_oracle.iaf_flow and not from a kernel:

    a0[b,m,:] = C[win[b], m, :] + theta_term[b, :] + sum_j u[b, s*m + j] * w_eps[j, :]          m < Lh, s = 1 | 2
    x_0 = elu(a0);  x_{l+1} = bn_l(elu(x_l W_l + b_l))                                          l < n_hidden
    (mu, r) = x_nh W_head + b_head;  sigma = softplus(r) + 1e-10
    stride 1: u_next[t] = u[t+k] sigma[t] + mu[t]
    stride 2: u_next[2m] = u[2m+k];  u_next[2m+1] = u[2m+1+k] sigma[m] + mu[m]
    logsig[b] = sum of log sigma over the last n_logsig outputs

bn_l(e) = gamma_l e BN_SCALE + beta_l is tf.layers.batch_normalization(training=False) with its initial moving
statistics (mean 0, variance 1, epsilon 1e-3): BN_SCALE = 1 / sqrt(1 + 1e-3).

swap_out and n_logsig.  The count runs over the UNSWAPPED interleaved sequence: output o (even o = 2m: the copy,
sigma = 1, log sigma = 0; odd o = 2m + 1: the head position m) is counted iff o >= Lout - n_logsig, and swap_out
only moves where output o is stored (to o ^ 1).  flow_v4.hip:466-474 does exactly this: the store index is
`a.swap_out ? (o ^ 1) : o`, the count tests the unswapped `o >= a.Lout - a.n_logsig`.  So under stride 2 an odd
n_logsig counts the same head positions as n_logsig - 1.

Rounding switches (the bars of the reduced precisions).  Every matrix product goes through
oracle.precision_model.BMM, which rounds to bf16 the operands the switches of precision_model.MODE name (fwd_x, fwd_w,
bwd_g, bwd_w, wg_x; `precision_model.emulate(mode, realisation)` sets them); with no switch on it is the exact
product.  For one hidden layer without BN at stride 1 this is operand for operand precision_model.iaf_flow_emul
(with EXTRA's points off).  The
rounding points, each with the kernel line that rounds it (viforssms_amd/csrc/flow_v5.hip):

  fwd_x  the u taps of the layer-0 product and every ELU output that feeds a product (the accumulators packed to bf16
         as the B operand: "activations are MFMA accumulators ... take the accumulators directly as the B operand",
         :17-23; put_image writes the same bf16 images for the weight-gradient products, :739)
  fwd_w  w_eps (prep_kernel WE, :409), the hidden weights (WF, :400) and the head weights (WH, :431), each written as
         (__bf16)v[j] at :440.  With BN the kernels see the FOLDED weights W~_l = diag(gamma_{l-1} BN_SCALE) W_l
         (wt_hid :340-343, wt_head :344-347) and the folded biases b~_l = b_l + W_l^T beta_{l-1} (bias_hid :350-355,
         bias_head :356-361); the folded bias sits in K row 63 of the same fragments (:397, :401, :432: "the folded
         bias rides in the MFMA") against a ones row of the activations (:730), so it is rounded to bf16 as a weight.
         The reference therefore forms W~ and b~ in float64 from (W, gamma, beta) and rounds the folded operands,
         bias row included; autograd through the folding is the exact unfolding scatter_wgrad_kernel applies in fp32
         (:3334-3380).  (Without BN the biases ride in row 63 too; the established one-hidden-layer model leaves them
         unrounded and so does this one.)
  bwd_g  the gradient operand of every backward-chain product (dI = W dZ, dcon = w_eps dA0, the head backward) and
         of every weight-gradient product; the window-shared dC and d theta_term sum the bf16 dA0 image (:1180, :3067
         against a ones operand; dc16 slab :3329)
  bwd_w  the backward chain's weights: the same folded values transposed (prep_kernel WB :402-405, WC :421-424, the
         head pairs in cst :452-458)
  wg_x   the weight-gradient products read the bf16 images of the activations, ones row included (:1334, :1347: the
         bias gradient is the ones row's product, so it sums the bf16 dZ: with BN that falls out of the folded
         product, without BN it is the point EXTRA["bias_g"] below, which iaf_flow_emul lacks)

C + theta_term enter as the fp32 accumulator's initial value (pad_kernel :466-472) and are not rounded; softplus, the
ELU and the output u sigma + mu are fp32.  Stride 2 changes which positions reach the head, not what is rounded.  The
split modes switch fwd_w (bf16x2f) and bwd_w (bf16x2) off: w_hi x + w_lo x is exact to ~2^-16; bf16x3 is exact-class.
"""
from __future__ import annotations

import math

import torch

from oracle import precision_model as PM

DT = torch.float64
BN_SCALE = 1.0 / math.sqrt(1.0 + 1e-3)   # batch_normalization(training=False): moving mean 0, variance 1, eps 1e-3
LOG_2PI = math.log(2.0 * math.pi)
# Rounding points beyond precision_model.iaf_flow_emul's (on by default; tests/test_flow_ref.py ties the two models
# with them off):
#   bias_g  the gradient of an unfolded bias is the ones row's weight-gradient product, so it sums the bf16-rounded dZ
#           (flow_v5.hip:1334 hidden, :1347 head), under the bwd_g switch -- at H = 1 nothing else masks it
EXTRA = {"bias_g": True}
WEIGHTS = ("w_eps", "w_hid", "b_hid", "bn_g", "bn_b", "w_head", "b_head")


def _elu(x):
    return torch.where(x > 0, x, torch.expm1(torch.clamp(x, max=0.0)))


def _mm_bias(x, W, b, folded):
    """x W + b through the rounding product; folded: the bias as K row of the product (against a ones column)."""
    if not folded:
        # the bias gradient sums the bf16 dZ image (EXTRA["bias_g"]); the forward bias stays unrounded
        return PM.BMM.apply(x, W) + (PM.GradRound.apply(b.expand(*x.shape[:-1], -1)) if EXTRA["bias_g"] else b)
    ones = torch.ones(*x.shape[:-1], 1, dtype=x.dtype)
    return PM.BMM.apply(torch.cat([x, ones], -1), torch.cat([W, b[None, :]], 0))


def flow_layers(u, C, win, theta_term, w_eps, w_hid, b_hid, bn_g, bn_b, w_head, b_head, *, k, n_hidden, bn, stride2,
                folded=None):
    """(mu, r, pre): head outputs [B, Lh] and the list of ELU pre-activations per layer (layer 0 first).
    folded: the BN affine folded into the consuming layer (the kernels' form); None: folded iff bn and a rounding
    switch is on."""
    s = 2 if stride2 else 1
    B, L = u.shape
    Lh = (L - k) // s
    if folded is None:
        folded = bool(bn) and any(PM.MODE.values())
    folded = bool(folded and bn and n_hidden > 0)
    U = u.unfold(1, k, 1)[:, 0:s * Lh:s, :][:, :Lh]                    # [B, Lh, k]: taps u[b, s m + j]
    Cw = C[win.long()] if win is not None else C[0][None].expand(B, -1, -1)
    a = PM.BMM.apply(U, w_eps) + PM.GradRound.apply(Cw + theta_term[:, None, :])
    pre = [a]
    h = _elu(a)
    for l in range(n_hidden):
        if folded:
            W = w_hid[l] * (bn_g[l - 1] * BN_SCALE)[:, None] if l > 0 else w_hid[l]
            b = b_hid[l] + bn_b[l - 1] @ w_hid[l] if l > 0 else b_hid[l]
            z = _mm_bias(h, W, b, True)
            h = _elu(z)
        else:
            z = _mm_bias(h, w_hid[l], b_hid[l], False)
            h = _elu(z)
            if bn:
                h = bn_g[l] * h * BN_SCALE + bn_b[l]
        pre.append(z)
    if folded:
        Wh = w_head * (bn_g[n_hidden - 1] * BN_SCALE)[:, None]
        bh = b_head + bn_b[n_hidden - 1] @ w_head
        head = _mm_bias(h, Wh, bh, True)
    else:
        head = _mm_bias(h, w_head, b_head, False)
    return head[..., 0], head[..., 1], pre


def flow_ref(u, C, win, theta_term, w_eps, w_hid, b_hid, bn_g, bn_b, w_head, b_head, *, k, n_hidden, bn, stride2,
             swap_out, n_logsig, folded=None, n_logsig_count=None):
    """(u_next [B, L - k], logsig [B]) of vissm_flow_fwd, float64 with autograd.  n_logsig_count: count this many
    outputs instead (the power test's miscount mutation)."""
    B, L = u.shape
    Lout = L - k
    mu, r, _ = flow_layers(u, C, win, theta_term, w_eps, w_hid, b_hid, bn_g, bn_b, w_head, b_head, k=k,
                           n_hidden=n_hidden, bn=bn, stride2=stride2, folded=folded)
    sig = torch.nn.functional.softplus(r) + 1e-10
    nls = n_logsig if n_logsig_count is None else n_logsig_count
    if stride2:
        Lh = Lout // 2
        tail = u[:, k:k + 2 * Lh].reshape(B, Lh, 2)
        un = torch.stack([tail[..., 0], tail[..., 1] * sig + mu], -1)          # [B, Lh, 2]: (copy, head)
        o = 2 * torch.arange(Lh) + 1                                            # unswapped index of head position m
        counted = (o >= Lout - nls).to(DT)
        if swap_out:
            un = un.flip(-1)
        un = un.reshape(B, Lout)
    else:
        un = u[:, k:] * sig + mu
        counted = (torch.arange(Lout) >= Lout - nls).to(DT)
        if swap_out:
            un = un.reshape(B, Lout // 2, 2).flip(-1).reshape(B, Lout)
    return un, (torch.log(sig) * counted).sum(1)


def _leaves(u, C, theta_term, ws):
    req = lambda t: t.detach().clone().requires_grad_(True) if t is not None else None
    return req(u), req(C), req(theta_term), [req(w) for w in ws]


def _grads(loss_terms, grad_outs, u, C, theta_term, ws):
    ins = [u, C, theta_term] + [w for w in ws if w is not None]
    gs = torch.autograd.grad(loss_terms, ins, grad_outs, allow_unused=True)
    gs = [g if g is not None else torch.zeros_like(t) for g, t in zip(gs, ins)]
    out = {"du": gs[0], "dC": gs[1], "dtheta_term": gs[2]}
    it = iter(gs[3:])
    for name, w in zip(WEIGHTS, ws):
        if w is not None:
            out["d" + name] = next(it)
    return out


def flow_ref_all(u, C, win, theta_term, ws, du_next, dlogsig, **cfg):
    """Every output of vissm_flow_fwd + vissm_flow_bwd for upstream gradients du_next (stored layout) and dlogsig:
    u_next, logsig, du, dC, dtheta_term and d<weight> for the seven weight tensors `ws` (bn_g / bn_b None without BN)."""
    u, C, theta_term, ws = _leaves(u, C, theta_term, ws)
    un, ls = flow_ref(u, C, win, theta_term, *ws, **cfg)
    out = {"u_next": un.detach(), "logsig": ls.detach()}
    out.update(_grads([un, ls], [du_next, dlogsig], u, C, theta_term, ws))
    return out


def ar_terms(x, theta, obs, obs_bin, obs_std):
    """(sde [B], obs [B]) of the AR(1) model over the path x [B, M + 1] (include/vissm.h, vissm_flow_ar_elbo_fused;
    AR.py:168-176): the transition x_{t+1} ~ N(theta_1 x_t + theta_0, exp(theta_2)) and the masked observation
    y_t ~ N(x_{t+1}, obs_std), obs / obs_bin [B, M] per sample."""
    x1, x0 = x[:, 1:], x[:, :-1]
    sd = torch.exp(theta[:, 2:3])
    z = (x1 - (theta[:, 1:2] * x0 + theta[:, 0:1])) / sd
    sde = (-0.5 * z * z - theta[:, 2:3] - 0.5 * LOG_2PI).sum(1)
    zo = (x1 - obs) / obs_std
    ob = ((-0.5 * zo * zo - math.log(obs_std) - 0.5 * LOG_2PI) * obs_bin).sum(1)
    return sde, ob


def fused_ref(u, C, win, theta_term, theta, obs, obs_bin, obs_std, scale, ws, **cfg):
    """The reference of vissm_flow_ar_elbo_fused: the flow with its output x fed to the AR(1) terms, for
    loss = -scale sum_b (sde_b + obs_b + logsig_b).  obs / obs_bin [n_win, M].  Returns x, logsig, du, dC,
    dtheta_term and the weight gradients of the loss (theta is a constant here: its gradient goes through x in a
    separate call)."""
    u, C, theta_term, ws = _leaves(u, C, theta_term, ws)
    x, ls = flow_ref(u, C, win, theta_term, *ws, **cfg)
    wl = win.long() if win is not None else torch.zeros(u.shape[0], dtype=torch.long)
    sde, ob = ar_terms(x, theta, obs[wl], obs_bin[wl], obs_std)
    loss = -scale * (sde + ob + ls).sum()
    out = {"x": x.detach(), "logsig": ls.detach()}
    out.update(_grads([loss], None, u, C, theta_term, ws))
    return out


# ---------------------------------------------------------------------------------------------------------------
# error measures and bars (tests/test_gpu_flow_abi.py; the CPU power test applies them to mutants)
# ---------------------------------------------------------------------------------------------------------------
ROWWISE = ("u_next", "x", "du", "dtheta_term")
FORWARD = ("u_next", "x", "logsig")


def _den(x):
    m = float(x.abs().max()) if x.numel() else 0.0
    return m if m > 0 else 1.0


def measure(name, got, ref):
    """The per-tensor error figure: rows (u_next, x, du, dtheta_term): max|got - ref| over the row / max|ref| over the
    row, worst row; logsig: |got - ref| / max_b|ref|; dC: max|got - ref| / max|ref| per window, worst window; a
    weight gradient: max|got - ref| / max|ref| over the tensor.  A zero reference row / tensor divides by 1."""
    got, ref = got.double(), ref.double()
    if ref.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    d = (got - ref).abs()
    if name in ROWWISE or name == "dC":
        d2, r2 = d.reshape(d.shape[0], -1), ref.abs().reshape(ref.shape[0], -1)
        den = r2.max(1).values
        den = torch.where(den > 0, den, torch.ones_like(den))
        return float((d2.max(1).values / den).max())
    return float(d.max()) / _den(ref)


def measures(got: dict, ref: dict) -> dict:
    return {n: measure(n, got[n], ref[n]) for n in ref if n in got}


FWD_BAR, GRAD_BAR = 1e-4, 1e-3     # parity_util.FP32_BAR: elbo_tol / grad_tol


def exact_bars(names) -> dict:
    return {n: (FWD_BAR if n in FORWARD else GRAD_BAR) for n in names}


def emulated_bars(run, mode, names, safety, realisations) -> dict:
    """safety x envelope + the fp32 bar (parity_util.emulated_tol's rule, per tensor): run() evaluates the reference's
    outputs under the current switches; the envelope is the maximum of measure() over `realisations` realisations of
    `mode` against the exact reference."""
    with PM.emulate(None):
        ref = run()
    env = {n: 0.0 for n in names}
    for r in range(realisations):
        with PM.emulate(mode, realisation=r):
            em = run()
        for n in names:
            env[n] = max(env[n], measure(n, em[n], ref[n]))
    ex = exact_bars(names)
    return {n: safety * env[n] + ex[n] for n in names}, ref
