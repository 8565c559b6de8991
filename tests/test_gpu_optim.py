"""optimisers.adamax.AdamaxOptimizer (the drop-in facade of optimisers/adamax.py:11-61) on the HIP kernels,
against the oracle's clip_by_global_norm + adamax_update (AR.py:230-234, optimisers/adamax.py:42-58)
over several steps: contiguous, non-contiguous (a transposed view) and fp16 variables in one call,
with and without the global-norm clip, and the in-place path for consecutive views of one buffer.

Below that, the kernels' own edges, called on raw buffers: vissm_sqnorm and AdamaxKernel.step at sizes where their
grid-stride loops make a second trip (n > 1024 * 1024 for the norm partials, n > 2048 * 256 for the update), from base
pointers that are not 16-byte aligned, at n = 0, and with a gradient whose norm overflows fp32 but not the double
the kernel sums in."""

import numpy as np
import pytest
import torch

from oracle import nma_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _oracle_steps(vals, grads_seq, lr, b1, b2, clip, eps):
    vals = [v.double().clone() for v in vals]
    slots = [(torch.zeros_like(v), torch.zeros_like(v)) for v in vals]
    for grads in grads_seq:
        gs = [g.double() for g in grads]
        if clip > 0:
            gs, _ = O.clip_by_global_norm(gs, clip)
        out = []
        for i, (v, g, (sv, sm)) in enumerate(zip(vals, gs, slots)):
            nv, nsv, nsm = O.adamax_update(v, g, sv, sm, lr, b1, b2, eps[i])
            out.append(nv)
            slots[i] = (nsv, nsm)
        vals = out
    return vals, slots


@pytest.mark.parametrize("clip", [0.0, 5.0])
def test_facade_mixed_layouts_and_dtypes(clip):
    from optimisers.adamax import AdamaxOptimizer
    g = torch.Generator().manual_seed(1)
    a = torch.randn(37, generator=g)
    base = torch.randn(6, 9, generator=g)
    h = torch.randn(11, generator=g).half()
    vars_ = [a.to(DEV), base.to(DEV).t(), h.to(DEV)]          # the second is a non-contiguous view
    assert not vars_[1].is_contiguous()
    init = [v.detach().float().cpu().clone() for v in vars_]
    opt = AdamaxOptimizer(learning_rate=1e-2, beta1=0.95)
    grads_seq = []
    for _ in range(3):
        grads = [torch.randn(v.shape, generator=g) * 3 for v in vars_]
        grads_seq.append(grads)
        opt.apply_gradients([(gr.to(DEV).to(v.dtype), v) for gr, v in zip(grads, vars_)], clip_norm=clip)
    torch.cuda.synchronize()
    grads_in = [[gr.to(v.dtype).float() for gr, v in zip(grads, vars_)] for grads in grads_seq]
    ref, slots = _oracle_steps(init, grads_in, 1e-2, 0.95, 0.999, clip, [1e-8, 1e-8, 1e-7])
    for i, (v, r) in enumerate(zip(vars_, ref)):
        tol = 2e-3 if v.dtype == torch.float16 else 1e-5
        assert torch.allclose(v.double().cpu(), r, rtol=tol, atol=tol), i
    for i, v in enumerate(vars_[:2]):
        assert torch.allclose(opt.get_slot(v, "v").double().cpu(), slots[i][0], rtol=1e-5, atol=1e-6)
        assert torch.allclose(opt.get_slot(v, "m").double().cpu(), slots[i][1], rtol=1e-5, atol=1e-6)


def test_facade_consecutive_views_update_in_place():
    from optimisers.adamax import AdamaxOptimizer
    flat = torch.randn(100, device=DEV)
    views = [flat[0:30].view(5, 6), flat[30:100]]
    copies = [v.clone() for v in views]
    g = [torch.randn_like(v) for v in views]
    o1, o2 = AdamaxOptimizer(1e-3, 0.9), AdamaxOptimizer(1e-3, 0.9)
    assert o1._group_for(views).flat_view is not None
    o1.apply_gradients(list(zip(g, views)), clip_norm=2.0)
    o2.apply_gradients(list(zip(g, copies)), clip_norm=2.0)
    torch.cuda.synchronize()
    assert o2._group_for(copies).flat_view is None
    for v, c in zip(views, copies):
        assert torch.equal(v, c)


def test_facade_slots_follow_changing_groupings():
    """var lists [a, b] -> [a] (b's gradient None) -> [a, b] again: the cached group of the first call must pick up
    a's slots from the second call (one slot pair per variable, optimisers/adamax.py:36-40) and get_slot must keep
    returning the live values; checked against a per-variable oracle Adamax."""
    from optimisers.adamax import AdamaxOptimizer
    g = torch.Generator().manual_seed(5)
    a0, b0 = torch.randn(13, generator=g), torch.randn(7, generator=g)
    a, b = a0.to(DEV), b0.to(DEV)
    opt = AdamaxOptimizer(learning_rate=1e-2, beta1=0.9)
    seq = [("ab", torch.randn(13, generator=g), torch.randn(7, generator=g)),
           ("a", torch.randn(13, generator=g), None),
           ("ab", torch.randn(13, generator=g), torch.randn(7, generator=g)),
           ("a", torch.randn(13, generator=g), None),
           ("ab", torch.randn(13, generator=g), torch.randn(7, generator=g))]
    for _, ga, gb in seq:
        opt.apply_gradients([(ga.to(DEV), a), (None if gb is None else gb.to(DEV), b)])
    torch.cuda.synchronize()
    ra, sa = _oracle_steps([a0], [[ga] for _, ga, _ in seq], 1e-2, 0.9, 0.999, 0.0, [1e-8])
    rb, sb = _oracle_steps([b0], [[gb] for _, _, gb in seq if gb is not None], 1e-2, 0.9, 0.999, 0.0, [1e-8])
    assert torch.allclose(a.double().cpu(), ra[0], rtol=1e-5, atol=1e-6)
    assert torch.allclose(b.double().cpu(), rb[0], rtol=1e-5, atol=1e-6)
    for var, slots in ((a, sa[0]), (b, sb[0])):
        assert torch.allclose(opt.get_slot(var, "v").double().cpu(), slots[0], rtol=1e-5, atol=1e-6)
        assert torch.allclose(opt.get_slot(var, "m").double().cpu(), slots[1], rtol=1e-5, atol=1e-6)


# ---- vissm_sqnorm ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1023, 1025, 2 ** 20 + 7, 3 * 2 ** 20 + 1])
def test_sqnorm_matches_float64_sum(n):
    """The squares are summed in double and cast once, so the result is the float64 sum to one fp32 rounding
    (rtol 2^-23); a base pointer 1, 2 or 3 floats off a 256-byte boundary never takes the float4 path."""
    from viforssms_amd import _lib
    lib = _lib.load()
    st = _lib.stream_handle(torch.device(DEV))
    g = torch.Generator(device=DEV).manual_seed(n + 1)
    big = torch.randn(n + 8, generator=g, device=DEV) * 3
    assert big.data_ptr() % 256 == 0
    wsz = lib.vissm_adamax_workspace_size(n)
    ws = torch.empty(wsz, dtype=torch.uint8, device=DEV)
    for off in (0, 1, 2, 3):
        x = big[off:off + n]
        out = torch.full((3,), -7.0, device=DEV)
        _lib.check(lib.vissm_sqnorm(big.data_ptr() + 4 * off, n, out.data_ptr() + 4, ws.data_ptr(), wsz, st),
                   "vissm_sqnorm")
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        ref = float((x.double() ** 2).sum().item())
        assert got[0] == -7.0 and got[2] == -7.0
        if n == 0:
            assert got[1] == 0.0 and not np.signbit(got[1])
        else:
            assert abs(float(got[1]) - ref) <= 2.0 ** -23 * ref, (n, off, float(got[1]), ref)


# ---- clip + Adamax at a second grid-stride trip, from unaligned views ---------------------------------------
N_BIG = 2 ** 20 + 7


def _offset_views(tensors):
    """each tensor copied into a view that starts one float past its allocation: 4-byte, not 16-byte aligned"""
    out = []
    for t in tensors:
        buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
        view = buf[1:]
        view.copy_(t.float())
        assert view.data_ptr() % 16 == 4
        out.append(view)
    return out


@pytest.mark.parametrize("clip", [0.0, 50.0])
def test_adamax_kernel_second_trip_unaligned_views(clip):
    from viforssms_amd.ops import AdamaxKernel
    g = torch.Generator().manual_seed(11)
    n = N_BIG
    p = torch.randn(n, generator=g, dtype=torch.float64)
    gr = torch.randn(n, generator=g, dtype=torch.float64) * 3
    v = torch.randn(n, generator=g, dtype=torch.float64) * 0.1
    m = torch.rand(n, generator=g, dtype=torch.float64) + 0.01
    p, gr, v, m = (t.float().double() for t in (p, gr, v, m))             # what the kernel is given, exactly
    k = AdamaxKernel(n, DEV)
    P, G, V, Mm = _offset_views((p, gr, v, m))
    gn = k.step(P, G, V, Mm, 1e-3, 0.95, 0.999, 1e-8, clip)
    torch.cuda.synchronize()
    gg = [gr]
    if clip > 0:
        gg, _ = O.clip_by_global_norm([gr], clip)
    rp, rv, rm = O.adamax_update(p, gg[0], v, m, 1e-3, 0.95, 0.999)
    assert abs(gn.item() - gr.norm().item()) <= 1e-5 * gr.norm().item()
    assert torch.allclose(P.double().cpu(), rp, rtol=1e-6, atol=1e-6)
    assert torch.allclose(V.double().cpu(), rv, rtol=1e-5, atol=1e-6)
    assert torch.allclose(Mm.double().cpu(), rm, rtol=1e-5, atol=1e-6)
    assert torch.equal(G.double().cpu(), gr)                              # the gradient is read only
    # the guarded step with a finite gradient: nothing skipped, bitwise the unguarded result
    k2 = AdamaxKernel(n, DEV)
    P2, G2, V2, M2 = _offset_views((p, gr, v, m))
    gn2 = k2.step(P2, G2, V2, M2, 1e-3, 0.95, 0.999, 1e-8, clip, guard=True)
    torch.cuda.synchronize()
    assert k2.skipped.item() == 0
    for a, b in ((P, P2), (V, V2), (Mm, M2), (gn, gn2)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_guarded_step_with_a_norm_that_overflows_fp32():
    """2^20 + 7 gradient entries of +-3e38: the squares sum to 9.4e82 in the double the kernel carries, the norm is
    3.07e41 -- finite as a double, infinite as a float.  What the kernel does, pinned here: the guard tests the double
    norm, so the step is not skipped (skipped stays 0) and applies with scale = clip / norm computed in double
    (1.6e-40, a subnormal float: about 17 significant bits, a relative 4e-6 on the scaled gradient, inside the bars
    below); only the reported fp32 norm is +inf.  The oracle's float64 clip + Adamax is the reference."""
    from viforssms_amd.ops import AdamaxKernel
    g = torch.Generator().manual_seed(12)
    n, clip = N_BIG, 50.0
    p = torch.randn(n, generator=g, dtype=torch.float64).float().double()
    sign = (torch.rand(n, generator=g) < 0.5).double() * 2 - 1
    gr = (sign * 3e38).float().double()
    v = (torch.randn(n, generator=g, dtype=torch.float64) * 0.1).float().double()
    m = (torch.rand(n, generator=g, dtype=torch.float64) + 0.01).float().double()
    norm64 = torch.sqrt((gr ** 2).sum()).item()
    assert np.isfinite(norm64) and norm64 > float(np.finfo(np.float32).max)
    k = AdamaxKernel(n, DEV)
    P, G, V, Mm = _offset_views((p, gr, v, m))
    gn = k.step(P, G, V, Mm, 1e-3, 0.95, 0.999, 1e-8, clip, guard=True)
    torch.cuda.synchronize()
    assert k.skipped.item() == 0
    assert gn.item() == float("inf")
    gg, gn_ref = O.clip_by_global_norm([gr], clip)
    assert torch.isfinite(gn_ref) and torch.isfinite(gg[0]).all()
    rp, rv, rm = O.adamax_update(p, gg[0], v, m, 1e-3, 0.95, 0.999)
    assert torch.isfinite(P).all() and torch.isfinite(V).all() and torch.isfinite(Mm).all()
    assert torch.allclose(P.double().cpu(), rp, rtol=1e-6, atol=1e-6)
    assert torch.allclose(V.double().cpu(), rv, rtol=1e-5, atol=1e-6)
    assert torch.allclose(Mm.double().cpu(), rm, rtol=1e-5, atol=1e-6)
