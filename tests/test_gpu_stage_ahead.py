"""The flow kernels with each unit's input windows staged one unit ahead (VISSM_STAGE_AHEAD: bwd2_kernel's flagship
variants and the AR bf16 forward issue the next unit's u windows -- and upstream-gradient windows -- as LDS-DMA loads
into the other of two window buffers), at the branches of that staging:

  one_unit         B = 2, M = 12, k = 8: one tile, one pair: the prologue's staging only, nothing staged ahead;
  ghost_tail       B = 3, M = 40, k = 8: a ghost partner in the second pair (its gradient-window row zeroed by a plain
                   store, no DMA into it), a partial last tile, clamped source addresses at the row's end;
  one_tile_chunks  B = 5, M = 37, k = 5 at one tile per t-chunk: the next unit is always the next pair and the item ends
                   after the group's last pair; halo joins, the fused variant's look-back tile;
  two_groups       B = 20, M = 24, k = 8: a second group (its items stage nothing across the group's edge);
  k16              B = 4, M = 48, k = 16: nu = 32 lanes of the forward's windows active.

All with H = 50 and three flows, through the bf16 stacks with the last flow fused and unfused.

Each case, as in tests/test_gpu_bwd2_tail.py: the per-sample ELBO and every variable's gradient against the float64
oracle within the precision's rounding-model bar (parity_util.emulated_tol, no bar of this file's own), and ELBO and
flat gradient bitwise equal between two runs of the same inputs (a window read ahead of its DMA would return the bytes
of two units earlier on some runs).  The oracle's ELBOs are finite and no variable's oracle gradient is exactly zero
at these shapes and draws (asserted on the reference, computed once per shape and shared by the two stacks)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.parity_util import (EMUL_REALISATIONS, build_model, emulated_tol, oracle_reference)  # noqa: E402
from viforssms_amd._lib import TRAIN_PRECISIONS as PREC  # noqa: E402

DEV = "cuda:0"
SHAPES = {  # B, M, k, H, chunk_tiles
    "one_unit": (2, 12, 8, 50, 0),
    "ghost_tail": (3, 40, 8, 50, 0),
    "one_tile_chunks": (5, 37, 5, 50, 1),
    "two_groups": (20, 24, 8, 50, 0),
    "k16": (4, 48, 16, 50, 0),
}
STACKS = {  # precision, fuse_last
    "bf16_fused": ("bf16", True),
    "bf16_unfused": ("bf16", False),
}
MODEL_SEED = 7
# Draws: chosen on the CPU from the rounding model alone, by the rule of tests/test_gpu_bwd2_tail.py: per shape the
# first seed from 18 upwards whose four-realisation ELBO envelope is not below the model's 24-realisation rms
# (scripts/stage_ahead_draws.py prints the figures).  The bar stays emulated_tol's.
DRAW_SEED = {"one_unit": 22, "ghost_tail": 18, "one_tile_chunks": 19, "two_groups": 18, "k16": 18}
_CASES = {}


def _case(shape, prec_name):
    """Model, injected draws, float64 oracle reference and rounding-model envelope of (shape, precision): built once."""
    key = (shape, prec_name)
    if key in _CASES:
        return _CASES[key]
    from oracle.precision_model import PRECISION_MODE, emulate
    B, M, k, H, chunk_tiles = SHAPES[shape]
    prec = PREC[prec_name]
    model = build_model("ar", B, M, k, 3, H, 3, 3, DEV, precision=prec, seed=MODEL_SEED)
    model.engine.chunk_tiles = chunk_tiles
    md, st = model.mdef, model.store
    batch = model.engine.make_batch(np.zeros(B, dtype=np.int64))
    g = torch.Generator().manual_seed(DRAW_SEED[shape])
    eps = torch.randn(B, md.kernel_ext, generator=g, dtype=torch.float64)
    x0 = torch.randn(B, md.P_theta, generator=g, dtype=torch.float64) * md.theta_base[1] + md.theta_base[0]
    elbo_ref, ref_g = oracle_reference(model, batch, eps, x0)
    assert np.isfinite(elbo_ref).all(), elbo_ref
    dead = [n for n in st.names() if not np.linalg.norm(ref_g[n]) > 0]
    assert not dead, f"oracle gradient exactly zero for {dead}: replace the case"
    gref = np.concatenate([ref_g[n].ravel() for n in st.names()])
    gnorm = np.linalg.norm(gref)
    errs, per_em = [], {n: 0.0 for n in st.names()}
    for r in range(EMUL_REALISATIONS):
        with emulate(PRECISION_MODE[prec], realisation=r):
            e_em, g_em = oracle_reference(model, batch, eps, x0)
        gem = np.concatenate([g_em[n].ravel() for n in st.names()])
        errs.append((float(np.max(np.abs(e_em - elbo_ref) / np.maximum(np.abs(elbo_ref), 1e-6))),
                     float(np.linalg.norm(gem - gref) / (gnorm + 1e-30))))
        for n in st.names():
            per_em[n] = max(per_em[n], float(np.linalg.norm(g_em[n] - ref_g[n]) /
                                             (np.linalg.norm(ref_g[n]) + 1e-6 * gnorm + 1e-30)))
    emul = {"mode": PRECISION_MODE[prec], "elbo_rel_err": max(e[0] for e in errs),
            "grad_rel_err": max(e[1] for e in errs), "per_param": per_em}
    _CASES[key] = dict(model=model, batch=batch, eps=eps.float().to(DEV).contiguous(), x0=x0.float().to(DEV),
                       elbo_ref=elbo_ref, ref_g=ref_g, gref=gref, gnorm=gnorm, tol=emulated_tol({"emul": emul}))
    return _CASES[key]


def _step(c):
    model = c["model"]
    out = model.elbo_step(c["batch"], 0, eps=c["eps"], x0_theta=c["x0"], apply=False)
    model.store.sync_grads()
    torch.cuda.synchronize()
    return out["elbo"].detach().double().cpu().numpy(), model.store.grad.detach().double().cpu().numpy().copy()


@pytest.mark.parametrize("stack", list(STACKS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_stage_ahead_matches_oracle_and_repeats_bitwise(shape, stack):
    prec_name, fuse = STACKS[stack]
    c = _case(shape, prec_name)
    model, st = c["model"], c["model"].store
    model.engine.fuse_last = fuse
    if fuse:
        assert model.engine.fused_ok(c["batch"], SHAPES[shape][0]), "the step would not take the fused path"
    elbo, grad = _step(c)
    elbo2, grad2 = _step(c)
    assert np.isfinite(elbo).all() and np.isfinite(grad).all()
    tol = c["tol"]
    e_elbo = float(np.max(np.abs(elbo - c["elbo_ref"]) / np.maximum(np.abs(c["elbo_ref"]), 1e-6)))
    ggpu = np.concatenate([grad[a:a + s] for a, s in (st.offsets[n] for n in st.names())])
    e_grad = float(np.linalg.norm(ggpu - c["gref"]) / (c["gnorm"] + 1e-30))
    per = {}
    for n in st.names():
        a, s = st.offsets[n]
        r = c["ref_g"][n].ravel()
        per[n] = float(np.linalg.norm(grad[a:a + s] - r) / (np.linalg.norm(r) + 1e-6 * c["gnorm"] + 1e-30))
    worst = max(per, key=per.get)
    print(shape, stack, "ELBO %.3e (bar %.3e) grad %.3e (bar %.3e) worst variable %s %.3e (bar %.3e)" % (
        e_elbo, tol["elbo_tol"], e_grad, tol["grad_tol"], worst, per[worst], tol["param_tol"][worst]))
    assert e_elbo < tol["elbo_tol"], e_elbo
    assert e_grad < tol["grad_tol"], e_grad
    bad = {n: (e, tol["param_tol"][n]) for n, e in per.items() if not e < tol["param_tol"][n]}
    assert not bad, bad
    assert np.array_equal(elbo, elbo2), "per-sample ELBO differs between two runs of the same inputs"
    assert np.array_equal(grad, grad2), "flat gradient differs between two runs of the same inputs"
