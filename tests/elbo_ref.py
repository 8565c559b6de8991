"""Per-element reference and comparator for the ELBO log-density kernels (elbo.hip) at the C ABI.  No GPU needed.

reference(model, case, dtype) evaluates oracle/nma_oracle.py's terms and torch autograd on the CPU, in float64 or in
float32, from inputs that were generated in float64 and rounded to fp32 ONCE (round_case): the kernel and both
reference runs receive the same numbers, so input rounding is in no error figure.

The comparator (compare / assert_close): for a kernel output k with the two reference runs r64 and r32,
    scale = max |r32 - r64|        (dz: over each trajectory's row; dtheta: per theta component over the batch;
                                    sde / obs / extra: over the batch)
and EVERY element must satisfy |k - r64| <= C scale + floor + tiny, where tiny = 2^-24 |r64| is the rounding of an exact
result to the fp32 output (what r32's own last rounding costs, which a lucky r32 does not show in a scale taken over
a handful of numbers).  The bar is what an fp32 evaluation of the same
formulas costs on that row: it does not loosen where terms cancel in one element only, and a single wrong element
cannot hide behind large neighbours the way it does in a norm over the batch.  A failure names the worst element's
trajectory, index and code path in the kernel (chunk / lane / iteration, or the element-wise tail).

Cases: typical_case reuses the generators of tests/test_gpu_elbo.py and tests/test_gpu_elbo_models.py; tails_case
spreads the inputs to where an fp32 kernel and a float64 reference part ways (LV softplus over both of its regimes,
SV exp several units either side of the typical log-volatility), under three conditions on the reference alone
(case_conditions): r32 / r64 finite, every scale > 0, and per row scale <= 1e-3 max |r64|."""
import math

import numpy as np
import torch

from oracle import nma_oracle as O
from tests.test_gpu_elbo import _case as _ar_case
from tests.test_gpu_elbo_models import _case as _model_case

MODELS = ("ar", "lv", "sv", "fhn")
ZD = {"ar": 1, "lv": 2, "sv": 1, "fhn": 2}          # stored z entries per time
P = {"ar": 3, "lv": 3, "sv": 4, "fhn": 5}
KV = 4                                               # elbo.hip kV / kArV: times per chunk
TINY = 1e-30
OUT_ROUND = 2.0 ** -24   # rounding an exact result to the fp32 output: |r64| 2^-24 at the most
C_DEFAULT = 4.0
EXTRA_FLOOR_LV = 1e-6   # float64 -log(-expm1(-x)) rounds softplus(-z) ~ e^-x to 0 at large x; the kernel keeps it
OUTPUTS = ("sde", "obs", "extra", "dz", "dtheta")
_TENSORS = ("z", "theta", "obs", "bin", "mask", "shift", "dim_one", "gs", "go", "ge")


def _f32(v: float) -> float:
    return float(np.float32(v))


def round_case(d: dict) -> dict:
    """Every float input rounded to fp32 once (kept as float64 tensors holding fp32 values), dt / obs_std too."""
    out = dict(d)
    for k in _TENSORS:
        if out.get(k) is not None:
            out[k] = out[k].float().double()
    out["dt"] = _f32(out["dt"])
    out["obs_std"] = _f32(out.get("obs_std", 1.0))
    return out


def typical_case(model: str, B: int, M: int, n_win: int, seed: int) -> dict:
    """The existing suites' inputs: populations near 100 (LV), log-volatility near -8 (SV), unit spread (FHN),
    10 +- 3 (AR)."""
    if model == "ar":
        z, theta, obs, obs_bin, win, gs, go = _ar_case(B, M, n_win, seed)
        d = {"z": z, "theta": theta, "obs": obs, "bin": obs_bin, "win": win, "gs": gs, "go": go, "ge": None,
             "dt": 1.0, "obs_std": 1.3}
    else:
        d = _model_case(model, B, M, n_win, seed)
        d["obs_std"] = 1.0
        if model == "sv":
            d["go"] = None
        if model != "lv":
            d["ge"] = None
    if model != "sv":
        # the last row observed in every window: a window with no observation at all (likely at M <= 3) has obs == 0
        # exactly in every run, which the comparator's scale cannot grade
        d["bin"] = d["bin"].clone()
        d["bin"][..., -1] = 1.0
    d["model"], d["M"], d["n_win"] = model, M, n_win
    return round_case(d)


def tails_case(model: str, B: int, M: int, n_win: int, seed: int) -> dict:
    """Inputs at the tails.  LV: each coordinate's z sweeps [-12, 120] smoothly along the path (softplus in both of its
    fp32 regimes, e^z and z + e^-z, and the crossover between), window 0 pins x_0 as the reference does, and a few
    mask entries are neither 0 nor 1 (the general transform and its ILDJ).  SV: log-volatility states over
    -8 +- 5 and theta at both ends (+- 3 sd) of the spread the typical cases draw from.  FHN / AR: three times the
    typical spread."""
    d = typical_case(model, B, M, n_win, seed)
    g = torch.Generator().manual_seed(seed + 7919)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    t = torch.arange(M + 1, dtype=torch.float64)
    if model == "lv":
        # one cycle over the path, or t / 512 of one on a shorter path: steps below one unit of z (a jump across the
        # range in one step makes a transition of 1e9 nats whose theta gradient cancels badly).  One coordinate per
        # trajectory (alternating) starts at the low end, so that every ILDJ sum is of order 10: a path wholly at
        # large x has extra ~ e^-x, below fp32's reach and graded by the floor alone
        cyc = min(1.0, (M + 1) / 512.0)
        phase = u(B, 1, 2)
        low = torch.arange(B) % 2
        phase[torch.arange(B), 0, low] *= 0.03
        # window 0 pins x_0 (mask 0, shift x0) as the reference's first window does, here at x0 = (100, 0.01): its
        # trajectories start next to the pin (z = 100 and softplus^-1(0.01) = -4.6), not a jump away from it
        in0 = d["win"].long() == 0
        phase[in0, 0, 0] = 0.3727
        phase[in0, 0, 1] = 0.0757
        d["shift"] = d["shift"].clone()
        d["shift"][0, :, 0] = torch.tensor([100.0, 0.01], dtype=torch.float64)
        sweep = 0.5 * (1.0 - torch.cos(2 * math.pi * (cyc * t.view(1, -1, 1) / (M + 1) + phase)))   # [B, M+1, 2]
        d["z"] = (-12.0 + 132.0 * sweep + 0.1 * r(B, M + 1, 2)).reshape(B, 2 * (M + 1))
        mask, shift = d["mask"].clone(), d["shift"]
        # (factors near 1 and no shift: x moves by a few percent, which is a small step at either end of the range)
        for w in range(n_win):
            for pos, mv, sv in ((M // 2, 0.97, 0.0), (M, 1.02, 0.0), (min(M, KV * 65 + 1), 0.9, 0.0)):
                if pos >= 1:
                    mask[w, (w + pos) % 2, pos] = mv
                    shift[w, (w + pos) % 2, pos] = sv
        d["mask"], d["shift"] = mask, shift
        d["obs"] = 60.0 + 40.0 * r(n_win, 2, M)
    elif model == "sv":
        d["z"] = -8.0 + 10.0 * (u(B, M + 1) - 0.5)
        centre = torch.tensor([0.001, -0.6, math.log(0.08), math.log(0.5)], dtype=torch.float64)
        sd = torch.tensor([0.01, 0.1, 0.1, 0.1], dtype=torch.float64)
        sign = torch.where(torch.rand(B, 4, generator=g) < 0.5, -1.0, 1.0).double()
        d["theta"] = centre + 3.0 * sd * sign
    elif model == "fhn":
        d["z"] = 3.0 * r(B, 2 * (M + 1))
        d["obs"] = 3.0 * r(n_win, 2, M)
    else:
        d["z"] = 10.0 + 9.0 * r(B, M + 1)
        d["obs"] = 10.0 + 9.0 * r(n_win, M)
    return round_case(d)


def terms(model: str, d: dict, z: torch.Tensor, theta: torch.Tensor):
    """(sde, obs, extra) per sample from the oracle's terms, in z's dtype."""
    dt_ = z.dtype
    w = d["win"].long()
    B = z.shape[0]
    c = lambda k: d[k].to(dt_)
    zero = torch.zeros(B, dtype=dt_)
    if model == "ar":
        sde, obs = O.ar_elbo_terms(z, theta, c("obs")[w], c("bin")[w], d["obs_std"])
        return sde, obs, zero
    if model == "lv":
        x, extra = O.lv_transform(z, c("mask")[w], c("shift")[w])
        sde, obs = O.lv_elbo_terms(x, theta, c("obs")[w], c("bin")[w], d["dt"])
        return sde, obs, extra
    if model == "sv":
        x = torch.stack([c("dim_one")[w], z * c("mask")[w] + c("shift")[w]], 1)
        return O.sv_elbo_terms(x, theta, d["dt"]), zero, zero
    x = z.reshape(B, -1, 2).transpose(1, 2)
    sde, obs = O.fhn_elbo_terms(x, theta, c("obs")[w], c("bin")[w], d["dt"])
    return sde, obs, zero


def reference(model: str, d: dict, dtype=torch.float64, g_sde="case", g_obs="case", g_extra="case",
              z_constant: bool = False) -> dict:
    """sde, obs, extra [B], dz [B, ZD (M + 1)] and dtheta [B, P] of g_sde . sde + g_obs . obs + g_extra . extra, by
    the oracle's terms and torch autograd in `dtype`; returned as float64.  The upstream gradients default to the
    case's (gs / go / ge); None is zero.  z_constant: dz is not taken (zeros)."""
    pick = lambda v, k: d.get(k) if isinstance(v, str) else v
    ups = [pick(g_sde, "gs"), pick(g_obs, "go"), pick(g_extra, "ge")]
    z = d["z"].to(dtype).clone().requires_grad_(not z_constant)
    th = d["theta"].to(dtype).clone().requires_grad_(True)
    vals = terms(model, d, z, th)
    loss = None
    for v, gup in zip(vals, ups):
        if gup is not None and v.requires_grad:
            loss = (v * gup.to(dtype)).sum() if loss is None else loss + (v * gup.to(dtype)).sum()
    dz, dth = torch.zeros_like(z), torch.zeros_like(th)
    if loss is not None:
        loss.backward()
        dz = z.grad if z.grad is not None else dz
        dth = th.grad if th.grad is not None else dth
    out = {"sde": vals[0], "obs": vals[1], "extra": vals[2], "dz": dz, "dtheta": dth}
    return {k: v.detach().double() for k, v in out.items()}


def scale_of(name: str, r32: torch.Tensor, r64: torch.Tensor) -> torch.Tensor:
    """max |r32 - r64|, broadcastable to the output: per row (dz), per component over the batch (dtheta), over the
    batch (per-sample values)."""
    e = (r32 - r64).abs()
    if name == "dz":
        return e.amax(1, keepdim=True)
    if name == "dtheta":
        return e.amax(0, keepdim=True)
    return e.amax().reshape(1)


SCALE_BATCH = 9   # trajectories the scales are taken over (the largest batch the GPU matrix runs)


def sub_batch(d: dict, B: int) -> dict:
    """The first B trajectories of a case."""
    out = dict(d)
    for k in ("z", "theta", "win", "gs", "go", "ge"):
        if out.get(k) is not None:
            out[k] = out[k][:B].clone()
    return out


def scales_of(r32: dict, r64: dict, B: int) -> dict:
    """Every output's scale from the references of a SCALE_BATCH-trajectory case, for a kernel run on its first B
    trajectories.  A maximum over one or two numbers (B = 1: ONE per-sample value, one theta gradient per component)
    is no estimate of what fp32 costs: r32 is within a tenth of an ulp of r64 there as often as not, and an honest
    kernel one ulp away then misses any C.  The per-sample values and dtheta therefore take their scale over the whole
    SCALE_BATCH-trajectory case the B rows come from, whatever B the kernel runs; dz keeps its own row's."""
    return {k: (scale_of(k, r32[k], r64[k])[:B] if k == "dz" else scale_of(k, r32[k], r64[k])) for k in OUTPUTS}


def code_path(model: str, M: int, flat_index: int, kernel: str = "onepass") -> str:
    """Where the kernels evaluate stored dz entry `flat_index` of a row: the element-wise tail, or a chunk of the
    chunk loop with its lane and iteration.  kernel: "onepass" (stream_onepass_kernel: chunks 1 .. (M + 1) / kV - 1),
    "bwd" (stream_bwd_kernel / ar_elbo_bwd_kernel: chunks 1 .. M / kV - 1)."""
    t = flat_index // ZD[model]
    nfull = (M + 1) // KV if kernel == "onepass" and model != "ar" else M // KV
    c = t // KV
    if c == 0 or c >= nfull:
        return f"t={t}: tail ({'first kV elements' if c == 0 else 'past the last full chunk'})"
    it, lane = divmod(c - 1, 64)
    note = ""
    if kernel == "onepass" and model != "ar":
        last = c == nfull - 1 or lane == 63
        note = ", deferred chunk" if last else ""
        if t % KV == KV - 1 and last:
            note += " (its deferred last element)"
        if lane == 0 and t % KV == 0:
            note += " (lane 0: carried left neighbour)"
    return f"t={t}: chunk {c}, iteration {it}, lane {lane}, element {t % KV} of the chunk{note}"


def compare(name: str, k: torch.Tensor, r64: torch.Tensor, r32: torch.Tensor, C: float = C_DEFAULT,
            floor: float = 0.0, against=None, scale=None) -> dict:
    """The worst element of |k - r64| against C scale + floor + tiny.  Returns {"ok", "ratio" (largest
    (|k - r64| - floor - tiny)+ / scale over elements, inf where scale is 0 and the error is not), "index", "err",
    "bar"}.  against: another kernel output to measure k's distance from instead of r64, under the same bar.  scale: the
    scale to use instead of scale_of(name, r32, r64) (taken over a larger batch that holds these rows: scales_of)."""
    k = k.detach().double().cpu().reshape(r64.shape)
    sc = (scale_of(name, r32, r64) if scale is None else scale).expand_as(r64)
    err = (k - (r64 if against is None else against.detach().double().cpu().reshape(r64.shape))).abs()
    err = torch.where(torch.isfinite(k), err, torch.full_like(err, math.inf))
    # the output is stored in fp32: half an ulp of |r64| is the error of an exact evaluation
    tiny = r64.abs() * OUT_ROUND + TINY
    bar = torch.where(sc > 0, C * sc, torch.zeros_like(sc)) + floor + tiny
    excess = (err - floor - tiny).clamp_min(0.0)
    ratio = torch.where(excess > 0, excess / sc, torch.zeros_like(sc))       # x / 0 = inf
    i = int(torch.argmax(torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)))
    idx = np.unravel_index(i, tuple(r64.shape)) if r64.dim() else ()
    return {"ok": bool((err <= bar).all()), "ratio": float(ratio.reshape(-1)[i]), "index": tuple(int(j) for j in idx),
            "err": float(err.reshape(-1)[i]), "bar": float(bar.reshape(-1)[i])}


def assert_close(name: str, k, r64, r32, model: str, M: int, C: float = C_DEFAULT, floor: float = 0.0,
                 kernel: str = "onepass", what: str = "", against=None, scale=None) -> float:
    """compare(), raising with the worst element's trajectory, index and code path.  Returns the worst ratio."""
    res = compare(name, k, r64, r32, C, floor, against, scale)
    if not res["ok"]:
        idx = res["index"]
        where = f"trajectory {idx[0]}" if idx else ""
        if name == "dz":
            where += f", entry {idx[1]}, {code_path(model, M, idx[1], kernel)}"
        elif name == "dtheta":
            where += f", component {idx[1]}"
        ref = "r64" if against is None else "other"
        raise AssertionError(f"{what} {model} M={M} {name}: |k - {ref}| = {res['err']:.3e} > bar {res['bar']:.3e} "
                             f"(ratio {res['ratio']:.2f}, C = {C}) at {where}")
    return res["ratio"]


def case_conditions(model: str, d: dict) -> dict:
    """The three conditions a case must meet for the bar to mean something, from the reference alone: r32 / r64 finite,
    every scale > 0, per row scale <= 1e-3 max |r64|.  Outputs that are identically zero for the model (obs of SV,
    extra outside LV) are left out.  Returns {"finite", "positive", "capped", "worst_cap"}."""
    r64, r32 = reference(model, d, torch.float64), reference(model, d, torch.float32)
    finite = all(bool(torch.isfinite(r[k]).all()) for r in (r64, r32) for k in OUTPUTS)
    positive, capped, worst = True, True, 0.0
    for k in OUTPUTS:
        if (k == "obs" and model == "sv") or (k == "extra" and model != "lv"):
            continue
        if k == "extra" and float(r64[k].abs().max()) < EXTRA_FLOOR_LV:
            continue   # LV at populations ~100: extra ~ e^-100 is 0 in both runs, graded by the absolute floor alone
        sc = scale_of(k, r32[k], r64[k])
        if k == "dz":
            mx = r64[k].abs().amax(1, keepdim=True)
        elif k == "dtheta":
            mx = r64[k].abs().amax(0, keepdim=True)
        else:
            mx = r64[k].abs().amax().reshape(1)
        positive = positive and bool((sc > 0).all())
        rel = float((sc / mx.clamp_min(1e-300)).max())
        worst = max(worst, rel)
        capped = capped and rel <= 1e-3
    return {"finite": finite, "positive": positive, "capped": capped, "worst_cap": worst}


# -------------------------------------------------------------------------------------------------
# guarded buffers: an output of n floats inside a larger buffer of sentinels, the in-range part NaN
# -------------------------------------------------------------------------------------------------
SENTINEL_BITS = 0x7FC0BEEF   # a quiet NaN with a payload (no kernel computes it)
GUARD = 32   # floats of sentinel either side (more than one 16-byte store past either end)


def guarded_layout(n: int, offset: int = 0):
    """(total, lo): the buffer's length and the output's first float; offset extra floats shift the output off
    16-byte alignment (the allocation itself is 256-byte aligned)."""
    lo = GUARD + offset
    return lo + n + GUARD, lo


def fill_guarded(buf_i32: torch.Tensor, lo: int, n: int):
    """Sentinels everywhere, NaN in [lo, lo + n) (buf viewed as int32)."""
    buf_i32.fill_(SENTINEL_BITS)
    buf_i32[lo:lo + n] = 0x7FC00000


def guard_violations(buf_i32: torch.Tensor, lo: int, n: int):
    """Indices relative to the output (negative: before it, >= n: past it) whose sentinel changed, bitwise."""
    b = buf_i32.detach().cpu()
    bad = torch.nonzero(b != SENTINEL_BITS).reshape(-1)
    bad = bad[(bad < lo) | (bad >= lo + n)]
    return [int(i) - lo for i in bad]
