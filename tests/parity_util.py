"""Parity harness: run one ELBO evaluation + gradient through the product (libvissm on the GPU)
and through the CPU oracle (float64) on identical injected inputs, and report the errors.

Used by tests/test_gpu_parity.py and __graft_entry__.smoke()."""
from __future__ import annotations

import os
import sys
from typing import Dict, Optional

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import nma_oracle as O  # noqa: E402
from oracle import bridge  # noqa: E402


def _ar_data(T: int, seed: int, impute: int = 1):
    from viforssms_amd.data import data_gen
    st = np.random.get_state()
    np.random.seed(seed)
    obs, ob, tt = data_gen(T, impute, 10.0, np.array([5.0, 0.5, 3.0]), 1.0, write=False)
    np.random.set_state(st)
    return obs.astype(np.float32), ob.astype(np.float32), tt.astype(np.float32)


def build_model(family: str, B: int, M: int, k: int, n_flows: int, H: int, n_layers: int, fw: int,
                device: str, T: Optional[int] = None, precision: int = 0, seed: int = 3,
                impute: Optional[int] = None, condition: bool = False):
    """A small model of the given family with a random (non-trivial) parameter draw.

    condition: divide each feature-branch input row by its channel's magnitude over the series.
    The reference's time channel grows to T (AR.py:139-140), so at T = 5000 a random draw sends the
    paths to |x| ~ 1e6 and the ELBO to ~1e10, where even an fp32 execution of the oracle is off by
    ~1e-4 relative: the config-length cases use this conditioned draw (a state like a trained
    model's) so that the 1e-4 bar measures the kernels, not the conditioning."""
    from viforssms_amd import _lib
    from viforssms_amd.vi_ssm import ThetaSpec
    rng = np.random.default_rng(seed)
    nd = [H] * n_layers
    if family == "ar":
        from viforssms_amd.ar import VI_SSM
        T = T or M
        obs, ob, tt = _ar_data(T, seed, impute=impute or (2 if T % 2 == 0 else 1))
        priors = [(0.0, 10.0)] * 3
        spec = ThetaSpec(5, [list(rng.permutation(3)) for _ in range(4)], 1.5, 0.5, "elu")
        model = VI_SSM(obs, 1.0, 10.0, spec, priors, T, B, k, M, nd, n_flows, fw, ob, tt, device=device,
                       precision=precision, init_seed=seed)
        raw = dict(obs=obs, ob=ob, tt=tt, fw=fw, T=T)
    elif family == "lv":
        from viforssms_amd.lv import VI_SSM, make_theta_spec
        from viforssms_amd.data import lv_data_gen
        T = T or M
        obs, ob, tt, _ = lv_data_gen(T, dt=0.1, obs_every=max(2, M // 4), seed=seed)
        priors = [(np.log(4.428 / 10), 1e-4), (np.log(0.029 / 10), 1e-4), (np.log(2.957 / 10), 1e-4)]
        spec = ThetaSpec(4, [list(rng.permutation(3)) for _ in range(3)], 0.0, 1.0, "elu")
        model = VI_SSM(obs, ob, tt, np.array([100.0, 100.0]), spec, priors, 0.1, T * 0.1, B, k, M, nd, T,
                       n_flows, fw, device=device, precision=precision, init_seed=seed)
        raw = dict(obs=obs, ob=ob, tt=tt, x0=np.array([100.0, 100.0]), dt=0.1, Tf=T * 0.1, target=T, fw=fw)
    elif family == "sv":
        from viforssms_amd.sv import VI_SSM
        from viforssms_amd.data import load_sv
        obs = load_sv()
        T = T or M
        obs = obs[: T + 1]
        priors = [(0.0, 10.0)] * 4
        spec = ThetaSpec(5, [list(rng.permutation(4)) for _ in range(4)], 0.0, 1.0, "relu")
        model = VI_SSM(obs, -8.5, spec, priors, 1.0, T, B, k, M, nd, T, n_flows, fw, device=device,
                       precision=precision, init_seed=seed)
        raw = dict(obs=obs, x0=-8.5, dt=1.0, Tf=float(T), target=T, fw=fw)
    elif family == "fhn":
        from viforssms_amd.fhn import VI_SSM
        from viforssms_amd.data import fhn_data_gen
        T = T or M
        obs, ob, tt, _ = fhn_data_gen(T, dt=0.1, obs_every=max(2, M // 6), seed=seed)
        priors = [(0.0, 10.0)] * 5
        spec = ThetaSpec(4, [list(rng.permutation(5)) for _ in range(3)], 0.0, 1.0, "elu")
        model = VI_SSM(obs, ob, tt, np.array([2.0, 3.0]), spec, priors, 0.1, T * 0.1, B, k, M, nd, T, n_flows,
                       fw, device=device, precision=precision, init_seed=seed)
        raw = dict(obs=obs, ob=ob, tt=tt, x0=np.array([2.0, 3.0]), dt=0.1, Tf=T * 0.1, target=T, fw=fw)
    else:
        raise ValueError(family)
    # perturb every variable (biases included) so all gradient paths are exercised
    vals = model.store.state_numpy()
    for name, v in vals.items():
        if name.startswith("theta/"):
            continue
        scale = 0.05 if "bias" in name or "beta" in name else 0.0
        vals[name] = v + scale * rng.standard_normal(v.shape)
        if "gamma" in name:
            vals[name] = v + 0.1 * rng.standard_normal(v.shape)
    for name, v in vals.items():
        if name.startswith("theta/") and name.endswith("bias"):
            vals[name] = 0.05 * rng.standard_normal(v.shape)
    if family == "lv":
        # LV paths live near the populations (~100); the reference pre-trains lf_sample towards 75
        # before the ELBO (lotka_volterra_partial.py:301).  Shift mu of the last two flows (between
        # them every coordinate is transformed once) so the ELBO is finite and well conditioned.
        nf = model.mdef.n_flows
        for i in range(max(0, nf - 2), nf):
            vals[f"flow{i}/head/bias"][0] += 60.0
    if condition:
        ts0 = model.engine.table.windows([0])[0]
        mag = np.maximum(1.0, np.abs(ts0).max(0))
        if family == "sv":
            mag = np.concatenate([mag, mag[:-2]])
        for i in range(model.mdef.n_flows):
            vals[f"flow{i}/feat0/kernel"] = vals[f"flow{i}/feat0/kernel"] / mag[:, None]
    model.store.load_numpy(vals)
    model.build_flow()
    model._oracle_raw = raw   # the raw series, for the oracle's own feature assembly
    return model


def pin_theta(model, target):
    """Put q(theta) at `target` (raw theta, e.g. sim_util.TRUE_THETA of the data's generator) and return the model.  A
    random draw's LV rates send every particle or trajectory out of the positive orthant at its first step, and a
    random AR theta_1 above 1 sends the particles so far from the data that no weight is left.  The last bijector's
    output is (z - shift) e^-ls, so a log-scale bias of 3 and a shift bias of -e^3 target give
    theta = target + e^-3 (z - ...)."""
    vals = model.store.state_numpy()
    name = f"theta/maf{model.mdef.n_maf - 1}/dense3/bias"
    bias = vals[name].copy()
    bias[0::2] = -np.exp(3.0) * np.asarray(target)
    bias[1::2] = 3.0
    vals[name] = bias
    model.store.load_numpy(vals)
    return model


# The product cases of the filter, smoother and adapted-filter tests: family -> (B, M, k, n_flows, H, n_layers, fw), T,
# precision, S (the shapes of tests/test_gpu_forecast.py), the filters and particles of the two filter tests, and the
# result's keys.
FILTER_CASES = {"ar": ((64, 30, 5, 2, 20, 3, 4), 150, 0, 1),
                "lv": ((32, 24, 4, 2, 16, 5, 3), 24, 1, 2)}
FILTER_KF, FILTER_NF = 8, 64
FILTER_KEYS = ("probs", "filter/loglik", "filter/theta", "filter/ll_inc", "filter/ess", "filter/mean", "filter/sd",
               "filter/n_valid", "filter/quantiles")
SMOOTH_KEYS = ("smooth/mean", "smooth/sd", "smooth/n_valid", "smooth/quantiles")


def filter_model(family: str, device: str = "cuda:0"):
    """The FILTER_CASES model of the family with q(theta) at its generator's parameters."""
    from tests.sim_util import TRUE_THETA
    shape, T, prec, _ = FILTER_CASES[family]
    model = build_model(family, *shape, device, T=T, precision=prec, seed=3)
    return pin_theta(model, TRUE_THETA[model.mdef.model_id])


FAMILY_SHAPE = {  # D (state dimension), n_hidden, BN, stride-2 interleaved head
    "ar": (1, 1, False, False), "sv": (1, 3, True, False), "lv": (2, 3, True, True), "fhn": (2, 3, True, True)}


def bench_geometry(family: str, precision: int, B: int, M: int, k: int, n_flows: int, H: int = 50) -> list:
    """The backward launch geometry (vissm_flow_geometry, which = 1) of every flow of a `family` model at
    batch B and window length M: what the benchmark's launch runs, for the parity cases that force it at a
    small batch through VissmFlowDesc.chunk_tiles.  Host modes (bf16x3f / bf16x2f) run their backward at
    bf16.  No GPU needed."""
    from viforssms_amd import _lib
    D, nh, bn, s2 = FAMILY_SHAPE[family]
    prec = _lib.HOST_MODES[precision][1] if precision in _lib.HOST_MODES else precision
    L = n_flows * k + D * M + D
    out = []
    for i in range(n_flows):
        d = _lib.FlowDesc(B, L, k, H, nh, int(bn), int(s2), int(D == 2 and i < n_flows - 1), D * M, 1, prec, 0)
        out.append(_lib.flow_geometry(d, 1))
        L -= k
    return out


def oracle_inputs(model, starts):
    """time_feats [B, kext, C] and the model-specific feeds for window starts `starts`, assembled by
    the oracle's own restatement of the reference's host code from the raw series (independent of
    viforssms_amd.features): AR.py:135-150 + 262-288, lotka_volterra_partial.py:185-204 + 366-386,
    SV_dense.py:159-185 + 304-328, fitz_nag_NVP.py:182-202 + 346-366."""
    md = model.mdef
    r = model._oracle_raw
    fam = md.family
    starts = np.asarray(starts, dtype=np.int64)
    ex = {}
    if fam == "ar":
        ts = O.ar_time_feats(r["obs"], r["ob"], r["tt"], md.n_flows, md.k, md.M, r["fw"], r["T"], starts)
    elif fam in ("lv", "fhn"):
        d = O.pair_time_feats(fam, r["obs"], r["ob"], r["tt"], r["x0"], r["dt"], r["Tf"], r["target"], md.n_flows,
                              md.k, md.M, r["fw"], starts)
        ts = d["time_feats"]
        ex["bin"] = d["bin"]
        if fam == "lv":
            ex["mask"], ex["shift"] = d["mask"], d["shift"]
    else:
        d = O.sv_time_feats(r["obs"], r["x0"], r["dt"], r["Tf"], r["target"], md.n_flows, md.k, md.M, r["fw"], starts)
        ts = d["time_feats"]
        ex = {"mask": d["mask"], "shift": d["shift"], "dim_one": d["dim_one"]}
    # feed_dict into the reference's float32 placeholders (DTYPE = tf.float32, AR.py:10) rounds every feed
    f32 = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), dtype=O.DT)
    return f32(ts), {k: f32(v) for k, v in ex.items()}


def _cast32(o):
    if isinstance(o, torch.Tensor):
        return o.float()
    if isinstance(o, dict):
        return {k: _cast32(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return type(o)(_cast32(v) for v in o)
    return o


def oracle_elbo_fp32(model, batch, eps: torch.Tensor, x0: torch.Tensor) -> np.ndarray:
    """The same oracle executed in float32 (as TF1's fp32 CPU path computes): its distance from the
    float64 result measures how well conditioned a case is."""
    md = model.mdef
    spec = bridge.spec_from_mdef(md, eps.shape[0])
    params = _cast32(bridge.oracle_params(model.store.state_numpy(), spec, model.engine.theta_dist.masks_np))
    ts, ex = oracle_inputs(model, batch.starts)
    with torch.no_grad():
        o = O.elbo(spec, params, model.engine.perms, x0.float(), eps.float(), ts.float(), _cast32(ex))
    return o["elbo"].double().numpy()


def oracle_elbo_rows(model, starts, eps: torch.Tensor, x0: torch.Tensor) -> np.ndarray:
    """The float64 oracle's per-sample ELBO (no gradient) for samples with window starts `starts` and
    injected draws eps [n, kernel_ext] / x0 [n, P_theta] (float64, CPU): a sample's ELBO depends on its
    own draws and window only, so a few rows of a large batch are checked one by one."""
    md = model.mdef
    spec = bridge.spec_from_mdef(md, eps.shape[0])
    params = bridge.oracle_params(model.store.state_numpy(), spec, model.engine.theta_dist.masks_np)
    ts, ex = oracle_inputs(model, starts)
    with torch.no_grad():
        o = O.elbo(spec, params, model.engine.perms, x0, eps, ts, ex)
    return o["elbo"].double().numpy()


def oracle_reference(model, batch, eps: torch.Tensor, x0: torch.Tensor):
    """The float64 oracle's per-sample ELBO and d sum(-ELBO) / d variable (by store name) for the
    model's current parameters, the batch's window starts and the injected eps / theta-base draws."""
    md = model.mdef
    B = eps.shape[0]
    st = model.store
    spec = bridge.spec_from_mdef(md, B)
    params = bridge.oracle_params(st.state_numpy(), spec, model.engine.theta_dist.masks_np)
    ts, inv_ex = oracle_inputs(model, batch.starts)
    leaves = O.param_leaves(params)
    for t in leaves:
        t.requires_grad_(True)
    o = O.elbo(spec, params, model.engine.perms, x0, eps, ts, inv_ex)
    (-o["elbo"]).sum().backward()
    ref_g = bridge.oracle_grads_by_name(params, [t.grad if t.grad is not None else torch.zeros_like(t)
                                                 for t in leaves], spec)
    return o["elbo"].detach().numpy(), ref_g


def run_parity_case(family: str, B: int, M: int, k: int, n_flows: int, H: int, n_layers: int, fw: int,
                    device: str = "cuda:0", T: Optional[int] = None, starts=None, precision: int = 0,
                    seed: int = 3, impute: Optional[int] = None, condition: bool = False,
                    fp32_yardstick: bool = False, step_path: bool = False, chunk_tiles: int = 0,
                    emulate: bool = False) -> Dict:
    """step_path: the product side runs the training step's gradient (VI_SSM.elbo_step without the
    Adamax apply: for AR at bf16 / bf16x3 the last flow fused with the ELBO terms) instead of
    forward + autograd backward.  chunk_tiles > 0 forces the flow kernels' tiles per t-chunk
    (VissmFlowDesc.chunk_tiles): the launch geometry of a larger batch at this batch.
    emulate: also evaluate the oracle under the precision's rounding model (oracle/precision_model.py: bf16 / bf16x2f
    / bf16x2) and return its errors against the exact oracle ("emul": the tolerance source of a reduced-precision
    case, emulated_tol)."""
    torch.cuda.set_device(torch.device(device))
    model = build_model(family, B, M, k, n_flows, H, n_layers, fw, device, T=T, precision=precision, seed=seed,
                        impute=impute, condition=condition)
    model.engine.chunk_tiles = int(chunk_tiles)
    md = model.mdef
    if starts is None:
        starts = np.zeros(B, dtype=np.int64)
    starts = np.asarray(starts, dtype=np.int64)
    batch = model.engine.make_batch(starts)
    g = torch.Generator().manual_seed(seed + 11)
    eps = torch.randn(B, md.kernel_ext, generator=g, dtype=torch.float64)
    x0 = torch.randn(B, md.P_theta, generator=g, dtype=torch.float64) * md.theta_base[1] + md.theta_base[0]

    # ---- product (GPU) ----
    st = model.store
    if step_path:
        out = model.elbo_step(batch, 0, eps=eps.float().to(device).contiguous(), x0_theta=x0.float().to(device),
                              apply=False)
    else:
        st.zero_grad()
        out = model.forward(batch, 0, eps=eps.float().to(device).contiguous(), x0_theta=x0.float().to(device))
        loss = (-out["elbo"]).sum()
        loss.backward()
    st.sync_grads()
    torch.cuda.synchronize()
    elbo_gpu = out["elbo"].detach().double().cpu().numpy()
    grads_gpu = {n: st.grad[a:a + s].double().cpu().numpy().reshape(st.tensors[n].shape)
                 for n, (a, s) in st.offsets.items()}

    # ---- oracle (CPU float64) ----
    elbo_ref, ref_g = oracle_reference(model, batch, eps, x0)

    elbo_err = float(np.max(np.abs(elbo_gpu - elbo_ref) / np.maximum(np.abs(elbo_ref), 1e-6)))
    fp32_err = None
    if fp32_yardstick:
        e32 = oracle_elbo_fp32(model, batch, eps, x0)
        fp32_err = float(np.max(np.abs(e32 - elbo_ref) / np.maximum(np.abs(elbo_ref), 1e-6)))
    gref = np.concatenate([ref_g[n].ravel() for n in st.names()])
    ggpu = np.concatenate([grads_gpu[n].ravel() for n in st.names()])
    gnorm = np.linalg.norm(gref)
    per = {}
    for n in st.names():
        r, q = ref_g[n], grads_gpu[n]
        per[n] = float(np.linalg.norm(q - r) / (np.linalg.norm(r) + 1e-6 * gnorm + 1e-30))
    emul = None
    if emulate:
        from oracle.precision_model import PRECISION_MODE, emulate as _emulate
        mode = PRECISION_MODE[precision]
        errs, per_em = [], {n: 0.0 for n in st.names()}
        for r in range(EMUL_REALISATIONS):   # the plain emulation and scaled-domain realisations (envelope)
            with _emulate(mode, realisation=r):
                e_em, g_em = oracle_reference(model, batch, eps, x0)
            gem = np.concatenate([g_em[n].ravel() for n in st.names()])
            errs.append((float(np.max(np.abs(e_em - elbo_ref) / np.maximum(np.abs(elbo_ref), 1e-6))),
                         float(np.linalg.norm(gem - gref) / (gnorm + 1e-30))))
            for n in st.names():
                per_em[n] = max(per_em[n], float(np.linalg.norm(g_em[n] - ref_g[n]) /
                                                 (np.linalg.norm(ref_g[n]) + 1e-6 * gnorm + 1e-30)))
        emul = {"mode": mode, "elbo_rel_err": max(e[0] for e in errs), "grad_rel_err": max(e[1] for e in errs),
                "grad_max_param_err": max(per_em.values()), "per_param": per_em}
    return {
        "fused": bool(step_path and model.engine.fused_ok(batch, B)),
        "elbo_rel_err": elbo_err,
        "grad_rel_err": float(np.linalg.norm(ggpu - gref) / (gnorm + 1e-30)),
        "grad_max_param_err": max(per.values()),
        "worst_param": max(per, key=per.get),
        "elbo_ref_mean": float(elbo_ref.mean()),
        "per_param": per,
        "finite": bool(np.isfinite(elbo_gpu).all() and np.isfinite(ggpu).all()),
        "elbo_rel_err_fp32_oracle": fp32_err,
        "emul": emul,
    }


# realisations of the rounding model per emulated case (plain + scaled-domain): the envelope a GPU realisation is
# held to
EMUL_REALISATIONS = 4
# a reduced-precision case passes when each error is within SAFETY x the rounding model's envelope + the fp32 bar
EMUL_SAFETY = 3.0
FP32_BAR = dict(elbo_tol=1e-4, grad_tol=1e-3, param_tol=2e-2)


# the measured bars these cases were held to before the rounding model (round 4, tests/test_gpu_parity.py at
# 8b018e3~1): the emulated bar may tighten them, never loosen them
EMUL_CAP = {"bf16": dict(elbo_tol=5e-3, grad_tol=5e-2, param_tol=2e-1),
            "bf16x2f": dict(elbo_tol=2e-3, grad_tol=5e-2, param_tol=2e-1),
            "bf16x2": dict(elbo_tol=2e-3, grad_tol=1e-2, param_tol=1e-1)}


def emulated_tol(res: Dict, safety: float = EMUL_SAFETY, cap: Optional[Dict] = None) -> Dict:
    """Tolerances of a reduced-precision case from its precision's rounding model (run_parity_case(emulate=True)):
    safety x the emulated error's envelope + the fp32 bar -- derived from the mode's arithmetic, not from a
    measurement of the kernels -- and never above the mode's earlier measured bar (EMUL_CAP, or `cap`).  param_tol
    is per variable (the emulated envelope of that variable's error)."""
    em = res["emul"]
    cap = cap or EMUL_CAP.get(em["mode"], dict(elbo_tol=np.inf, grad_tol=np.inf, param_tol=np.inf))
    return dict(elbo_tol=min(cap["elbo_tol"], safety * em["elbo_rel_err"] + FP32_BAR["elbo_tol"]),
                grad_tol=min(cap["grad_tol"], safety * em["grad_rel_err"] + FP32_BAR["grad_tol"]),
                param_tol={n: min(cap["param_tol"], safety * v + FP32_BAR["param_tol"])
                           for n, v in em["per_param"].items()})
