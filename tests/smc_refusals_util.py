"""The refusals of the sequential Monte Carlo wrappers (ops.sde_simulate .. ops.sv_cpmmh and the six particle methods
of PosteriorDiagnostics) as a table: tests/golden/smc_refusals.json holds, per case, the function, the keyword
arguments that override a valid call's, the exception's class name and its whole message.  test_smc_refusals_host.py
(CPU tensors) and test_gpu_smc_refusals.py (what sits behind the GPU check) replay the table and compare both.

The table is a recording, never an expectation written by hand: run as a script, this file replays its case lists
against the tree it runs in and writes what that tree raises.  It is regenerated only at a commit whose refusals are
known to be right -- it was recorded at the commit before the wrappers came to share their bodies -- and a re-run on
any later tree must reproduce it byte for byte.

    python -m tests.smc_refusals_util [--out FILE.json]

The "host" section needs no GPU.  The "gpu" section is recorded where torch sees a GPU and otherwise carried over
from the file as it stands.  No case launches a kernel: every one ends in a refusal.

A value in a case's kwargs is a plain scalar or a tensor spec {"t": shape, "dtype": "f32" | "f64" | "i32" | "i64",
"cpu": true (on the host whatever the section), "nc": true (a strided view), "fill": value}.  The valid call of a
function is base_args(): K = C = 2, N = 64, T = 8."""
import argparse
import json
import os
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "smc_refusals.json")
DTYPES = {"f32": torch.float32, "f64": torch.float64, "i32": torch.int32, "i64": torch.int64}
K, N, T, M = 2, 64, 8, 64
INF, NAN = float("inf"), float("nan")


def tensor(spec, dev):
    shape = list(spec["t"])
    dev = "cpu" if spec.get("cpu") else dev
    dtype = DTYPES[spec.get("dtype", "f32")]
    if spec.get("nc"):
        shape[-1] *= 2
    x = torch.full(shape, spec.get("fill", 0), dtype=dtype, device=dev)
    return x[..., ::2] if spec.get("nc") else x


def t(*shape, **kw):
    return {"t": list(shape), **kw}


def base_args(fn, dev):
    """The keyword arguments of a call of ops.<fn> that no wrapper refuses (AR for the three-family functions)."""
    from viforssms_amd import _lib
    P = _lib.MODEL_P[_lib.MODEL_AR]
    z = lambda *shape, **kw: tensor(t(*shape, **kw), dev)
    rng = dict(seed=1, row0=0)
    ar = dict(model_id=_lib.MODEL_AR, obs=z(1, T, fill=1), obs_bin=z(1, T, fill=1), dt=0.1, obs_std=0.5)
    chain = dict(theta_cur=z(K, P), ll_cur=z(K, dtype="f64"), prior=z(P, 2, fill=1), x_start=z(1), N=N, n_iter=1, **rng)
    sv_chain = dict(theta_cur=z(K, 4), ll_cur=z(K, dtype="f64"), prior=z(4, 2, fill=1), h_start=z(1),
                    obs=z(T + 1, fill=1), dt=1.0, N=N, n_iter=1, **rng)
    return {
        "sde_simulate": lambda: dict(model_id=_lib.MODEL_AR, theta=z(K, P), x_start=z(K, 1), H=T, dt=0.1, **rng),
        "particle_filter": lambda: dict(ar, theta=z(K, P), x_start=z(1), N=N, **rng),
        "particle_smooth": lambda: dict(model_id=_lib.MODEL_AR, theta=z(K, P), cloud=z(K * N, 1, T), dt=0.1,
                                        M=M, **rng),
        "sv_filter": lambda: dict(theta=z(K, 4), x_start=z(1), obs=z(T + 1, fill=1), dt=1.0, N=N, **rng),
        "sv_smooth": lambda: dict(theta=z(K, 4), cloud=z(K * N, 1, 4), obs=z(T + 1, fill=1), dt=1.0, M=M, **rng),
        "pmmh": lambda: dict(ar, **chain, prop_chol=z(P, P)),
        "pmmh_adaptive": lambda: dict(ar, **chain, chol_in=z(K, P, P), adapt_end=1),
        "sv_pmmh": lambda: dict(sv_chain, prop_chol=z(4, 4)),
        "sv_pmmh_adaptive": lambda: dict(sv_chain, chol_in=z(K, 4, 4), adapt_end=1),
        "sv_filter_sorted": lambda: dict(theta=z(K, 4), x_start=z(1), obs=z(T + 1, fill=1), dt=1.0, N=N,
                                         aux_n=z(K, 2, N, 4), aux_r=z(K, T)),
        "sv_cpmmh": lambda: dict(sv_chain, chol_in=z(K, 4, 4), rho=0.9, aux_n=z(K, 2, 2, N, 4), aux_r=z(K, 2, T),
                                 aux_sel=z(K, dtype="i32")),
        "cpm_fresh_aux": lambda: dict(C=K, T=T, N=N, seed=1, row0=0, device=dev),
    }[fn]()


def stub(family="ar", T=20, p_local=64, bad=None, bad_at=0):
    """A PosteriorDiagnostics with just what its refusals read (the Stub of test_cpm_host.py): the series y[0 .. T] is
    linspace(1, 2) with y[bad_at] = bad.  No engine stands behind it, so a call that passes every refusal ends in an
    AttributeError, which no case records."""
    from viforssms_amd import _lib
    from viforssms_amd.diagnostics import PosteriorDiagnostics

    class Stub(PosteriorDiagnostics):
        def target_len(self):
            return T

    model_id = {"ar": _lib.MODEL_AR, "lv": _lib.MODEL_LV, "fhn": _lib.MODEL_FHN, "sv": _lib.MODEL_SV}[family]
    s = Stub()
    S = _lib.MODEL_S[model_id]
    s.mdef = types.SimpleNamespace(model_id=model_id, family=family)
    s.engine = types.SimpleNamespace(device="cpu", seed=1)
    s.p_local, s.x0 = p_local, 0.0
    s.obs = np.linspace(1.0, 2.0, T + 1)
    if bad is not None:
        s.obs[bad_at] = float(bad)
    s.filter_data = None
    if family != "sv":
        s._keep_filter_data(np.ones((S, T)), np.ones((S, T)), np.ones(S))
    return s


def run_case(case, dev):
    """Call the case's function; the exception it raises."""
    fn, kwargs = case["fn"], {k: tensor(v, dev) if isinstance(v, dict) else v for k, v in case["kwargs"].items()}
    try:
        if fn.startswith("diag."):
            getattr(stub(**case.get("stub", {})), fn[5:])(**kwargs)
        else:
            from viforssms_amd import ops
            getattr(ops, fn)(**{**base_args(fn, dev), **kwargs})
    except AttributeError:
        raise
    except Exception as e:  # noqa: BLE001 - the class is what the table records
        return e
    raise AssertionError(f"{fn}({case['kwargs']}) was not refused")


# ----------------------------------------------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------------------------------------------
def _ops(fn, *kwargs_list):
    return [{"fn": fn, "kwargs": kw} for kw in kwargs_list]


def _diag(fn, stub, *kwargs_list):
    return [{"fn": "diag." + fn, "stub": stub, "kwargs": kw} for kw in kwargs_list]


def host_cases():
    """Every refusal CPU tensors reach.  {} is the valid call on CPU tensors (GPU only); a case with two faults pins
    which one is reported."""
    from viforssms_amd import _lib
    SV, P = _lib.MODEL_SV, _lib.MODEL_P[_lib.MODEL_AR]
    iters = [dict(n_iter=-1), dict(it0=-1), dict(it0=2 ** 31 - 1), dict(it0=2 ** 31 - 1, N=96)]
    rows = [dict(row0=-1), dict(row0=2 ** 64)]
    adapt = [dict(adapt_end=-1), dict(adapt_end=2 ** 31), dict(target_accept=0.0), dict(target_accept=1.0),
             dict(target_accept=NAN), dict(gamma=0.0), dict(gamma=1.5), dict(gamma=NAN)]
    bad_n = [dict(N=n) for n in (0, 32, 96, 2048)]
    bad_dt = [dict(dt=v) for v in (0.0, -1.0, NAN, INF)]
    c = []
    c += _ops("sde_simulate", {}, dict(model_id=7), dict(model_id=-1), dict(row0=-1), dict(H=-1))
    c += _ops("particle_filter", {}, dict(proposal="auxiliary"), dict(proposal="adapted", obs_std=0.0),
              dict(proposal="adapted", obs_std=INF), dict(proposal="adapted", obs_std=NAN), dict(obs_std=0.0),
              dict(model_id=7), dict(model_id=SV), dict(model_id=SV, N=96), *bad_n,
              dict(N=96, theta=t(K, P, dtype="f64")),
              dict(theta=t(K, P, dtype="f64")), dict(theta=t(K, P + 1)), dict(dt=0.0), dict(row0=-1), dict(H=-1))
    c += _ops("particle_smooth", {}, dict(model_id=7), dict(model_id=SV), dict(M=32), dict(row0=-1),
              dict(cloud=t(K * 96, 1, T)))
    c += _ops("sv_filter", {}, *bad_n, *bad_dt, dict(N=96, dt=0.0), dict(theta=t(K, 3)),
              dict(obs=t(T + 1, dtype="f64")),
              dict(row0=-1), dict(H=-1))
    c += _ops("sv_smooth", {}, dict(dt=0.0), dict(M=32), dict(theta=t(K, 3)), dict(row0=-1))
    for fn in ("pmmh", "pmmh_adaptive"):
        c += _ops(fn, {}, dict(model_id=SV), dict(model_id=7), dict(model_id=SV, N=96), *bad_n,
                  *[dict(obs_std=v) for v in (0.0, -1.0, NAN, INF)], dict(N=96, obs_std=0.0), dict(dt=0.0),
                  dict(theta_cur=t(K, P + 1)), dict(theta_cur=t(P)), dict(theta_cur=t(0, P)),
                  dict(theta_cur=t(K, P + 1), n_iter=-1), *iters, dict(obs=t(T)), dict(obs=t(2, T)),
                  dict(obs_bin=t(1, T - 1)), dict(obs=t(1, T, dtype="f64")), *rows, dict(row0=-1, obs=t(T)),
                  dict(theta_cur=t(K, P, dtype="f64")), dict(ll_cur=t(K, dtype="f32")), dict(prior=t(P, 3)),
                  dict(x_start=t(2)))
    c += _ops("pmmh", dict(prop_chol=t(P, P + 1)), dict(prop_chol=t(P, P, dtype="f64")))
    for fn in ("sv_pmmh", "sv_pmmh_adaptive", "sv_cpmmh"):
        c += _ops(fn, {}, *bad_n, *bad_dt, dict(N=96, dt=0.0), dict(theta_cur=t(K, 3)), dict(theta_cur=t(4)),
                  dict(theta_cur=t(0, 4)), dict(theta_cur=t(K, 3), n_iter=-1), *iters, dict(obs=t(1, T + 1)),
                  dict(obs=t(0)), dict(obs=t(T + 1, dtype="f64")), dict(obs=t(T + 1, dtype="i32")), *rows,
                  dict(row0=-1, obs=t(1, T + 1)), dict(theta_cur=t(K, 4, dtype="f64")), dict(ll_cur=t(K, dtype="f32")),
                  dict(prior=t(4, 3)), dict(h_start=t(2)))
    c += _ops("sv_pmmh", dict(prop_chol=t(4, 5)))
    for fn in ("pmmh_adaptive", "sv_pmmh_adaptive", "sv_cpmmh"):
        Pf = P if fn == "pmmh_adaptive" else 4
        c += _ops(fn, *adapt, dict(adapt_end=-1, n_iter=-1), dict(adapt_end=-1, row0=-1),
                  dict(chol_in=t(K, Pf, Pf + 1)),
                  dict(chol_in=t(Pf, Pf)), dict(chol_in=t(K, Pf, Pf, dtype="f64")),
                  dict(chol_in=t(K, Pf, Pf + 1), row0=-1))
    c += _ops("sv_cpmmh", *[dict(rho=v) for v in (1.0, -0.1, NAN, INF, 1.0 - 1e-9)], dict(rho=1.0, dt=0.0),
              dict(rho=1.0, theta_cur=t(K, 3)), dict(aux_sel=t(K, dtype="i32", fill=2)), dict(aux_n=t(K, 2, 2, N, 5)))
    c += _ops("sv_filter_sorted", {}, *bad_n, *bad_dt, dict(N=96, dt=0.0), dict(theta=t(K, 3)), dict(obs=t(1)),
              dict(aux_n=t(K, 2, N, 5)))
    c += _ops("cpm_fresh_aux", dict(C=0), dict(T=0), dict(N=96), dict(row0=-1), dict(row0=2 ** 64 - K * (N + 1)))

    ar, sv = dict(family="ar"), dict(family="sv")
    sizes = [dict(n_particles=96), dict(n_theta=0), dict(n_theta=65), dict(n_particles=96, n_theta=0),
             dict(probs=[]), dict(probs=[0.5, 1.5]), dict(chunk=0), dict(chunk=-3), dict(n_theta=65, chunk=0)]
    paths = [dict(n_paths=32), dict(n_paths=96), dict(n_paths=2048), dict(n_paths=32, n_particles=96),
             dict(n_paths=32, chunk=0)]
    big = dict(n_theta=4096, n_particles=1024)
    for fn in ("particle_filter", "particle_smoother"):
        c += _diag(fn, ar, dict(proposal="auxiliary"), *sizes)
        c += _diag(fn, dict(family="lv"), dict(n_particles=96))
        c += _diag(fn, sv, {}, dict(proposal="auxiliary"), dict(n_particles=96))
    c += _diag("particle_smoother", ar, *paths)
    c += _diag("particle_smoother", dict(family="ar", T=0), {}, dict(n_paths=32))
    c += _diag("particle_smoother", dict(family="ar", T=1000, p_local=4096), big)
    series = [dict(family="sv", bad=NAN, bad_at=3), dict(family="sv", bad=INF, bad_at=20),
              dict(family="sv", bad=0.0, bad_at=5)]
    for fn in ("volatility_filter", "volatility_smoother"):
        c += _diag(fn, sv, *sizes)
        for fam in ("ar", "lv", "fhn"):
            c += _diag(fn, dict(family=fam), {}, dict(n_particles=96))
        for stub in series:
            c += _diag(fn, stub, {}, dict(chunk=0))
        c += _diag(fn, dict(family="sv", bad=0.0, bad_at=20), dict(n_particles=96))   # y[T] = 0 alone is no refusal
    c += _diag("volatility_smoother", sv, *paths)
    c += _diag("volatility_smoother", dict(family="sv", T=0), {}, dict(n_paths=32))
    c += _diag("volatility_smoother", dict(family="sv", T=1000, p_local=4096), big)
    c += _diag("volatility_smoother", series[0], dict(n_paths=32))
    mcmc = [dict(n_particles=96), dict(n_chains=0), dict(n_chains=65), dict(n_iter=10, burn_in=10), dict(burn_in=-1),
            dict(step_scale=0.0), dict(step_scale=INF), dict(step_scale=NAN), dict(probs=[]),
            dict(n_particles=96, n_chains=0), dict(adapt=True, burn_in=0), dict(adapt=True, target_accept=0.0),
            dict(adapt=True, target_accept=1.0), dict(adapt=True, adapt_decay=0.0), dict(adapt=True, adapt_decay=1.5),
            dict(target_accept=0.0, n_particles=96), dict(adapt=True, burn_in=0, target_accept=0.0)]
    c += _diag("theta_mcmc", ar, *mcmc, dict(correlation=0.99), dict(correlation=NAN),
               dict(correlation=0.5, n_particles=96))
    c += _diag("theta_mcmc", sv, {}, dict(correlation=0.99), dict(n_particles=96))
    c += _diag("volatility_mcmc", sv, *mcmc, *[dict(correlation=v) for v in (-0.1, 1.0, 0.99995, NAN, INF)],
               dict(correlation=0.99, n_particles=96), dict(correlation=1.0, n_particles=96))
    for fam in ("ar", "lv", "fhn"):
        c += _diag("volatility_mcmc", dict(family=fam), {}, dict(correlation=1.0), dict(n_particles=96))
    for stub in series:
        c += _diag("volatility_mcmc", stub, {}, dict(correlation=0.9), dict(n_particles=96))
    return c


def gpu_cases():
    """The refusals behind the GPU check: shapes, devices, the layout of loglik_in / ll_cur / x_next / aux_*, horizons
    and the values of aux_sel, every other argument valid and on the GPU."""
    from viforssms_amd import _lib
    SV, P = _lib.MODEL_SV, _lib.MODEL_P[_lib.MODEL_AR]
    rows = [dict(row0=-1), dict(row0=2 ** 64)]

    def vec(name, n, dtype="f64", other="f32"):
        """A contiguous [n] GPU vector of dtype is expected."""
        return [{name: t(n, dtype=dtype, cpu=True)}, {name: t(n, dtype=other)}, {name: t(n + 1, dtype=dtype)},
                {name: t(n, dtype=dtype, nc=True)}, {name: t(n, 1, dtype=dtype)}]

    def xnext(S):
        return [dict(x_next=t(K * M, S, cpu=True)), dict(x_next=t(K * M, S, dtype="f64")), dict(x_next=t(K * M - 1, S)),
                dict(x_next=t(K * M, S + 1)), dict(x_next=t(K * M, S, nc=True)), dict(x_next=t(K * M))]

    c = []
    c += _ops("sde_simulate", dict(theta=t(K, P, dtype="f64")), dict(theta=t(K, P, dtype="i32")),
              dict(x_start=t(K, 1, dtype="i32")), dict(theta=t(K, P, nc=True)), dict(theta=t(K, P + 1)),
              dict(theta=t(P)),
              dict(x_start=t(K + 1, 1)), dict(x_start=t(K, 2)), dict(x_start=t(K, 1, cpu=True)),
              dict(model_id=SV, theta=t(K, 4), x_start=t(K, 2), obs_std=1.0), dict(H=-1), dict(t0=-1),
              dict(t0=2 ** 31 - 4), dict(obs_std=1.0, t0=2 ** 30 - 4), *rows)
    c += _ops("particle_filter", *[{n: t(*s, dtype="i32")} for n, s in (("theta", (K, P)), ("x_start", (1,)),
                                                                         ("obs", (1, T)), ("obs_bin", (1, T)))],
              dict(theta=t(K, P, dtype="f64")), dict(obs=t(1, T, cpu=True)), dict(obs=t(1, T, nc=True)),
              dict(theta=t(K, P + 1)), dict(theta=t(P)), dict(theta=t(2 ** 21, P), N=1024), dict(x_start=t(K * N + 1,
              1)),
              dict(x_start=t(K * N, 2)), dict(x_start=t(2)), dict(x_start=t(K * N)), dict(x_start=t(K * N, 1, 1)),
              dict(obs=t(2, T)), dict(obs=t(T)), dict(obs_bin=t(1, T - 1)), dict(obs_bin=t(T)),
              dict(H=T + 1), dict(H=-1), dict(t0=-1), dict(t0=T + 1), dict(t0=4, H=5), *rows, dict(row0=-1, H=-1),
              *vec("loglik_in", K), dict(proposal="adapted", loglik_in=t(K, dtype="f32")),
              dict(theta=t(K, P + 1), x_start=t(3)), dict(H=-1, loglik_in=t(K, dtype="f32")))
    c += _ops("particle_smooth", dict(theta=t(K, P, dtype="i32")), dict(cloud=t(K * N, 1, T, dtype="i32")),
              dict(theta=t(K, P + 1)), dict(theta=t(0, P)), dict(theta=t(P)), dict(cloud=t(K * N, T)),
              dict(cloud=t(K * N, 2, T)), dict(cloud=t(K * N - 1, 1, T)), dict(cloud=t(K * N, 1, T, nc=True)),
              dict(cloud=t(K * 96, 1, T)), dict(M=32), dict(M=96), dict(M=128), dict(M=0),
              dict(theta=t(65536, P), cloud=t(65536 * N, 1, 1)), dict(cloud=t(K * N, 1, 0)), dict(t0=-1),
              dict(t0=2 ** 31 - T), *rows, *xnext(1), dict(M=32, t0=-1), dict(t0=-1, x_next=t(K * M)))
    c += _ops("sv_filter", dict(theta=t(K, 4, dtype="i32")), dict(x_start=t(1, dtype="i32")),
              dict(theta=t(K, 4, dtype="f64")), dict(theta=t(K, 3)), dict(theta=t(4)), dict(theta=t(2 ** 21, 4),
              N=1024),
              dict(x_start=t(3)), dict(x_start=t(K * N + 1)), dict(x_start=t(K * N, 1, 1)),
              dict(obs=t(T + 1, cpu=True)), dict(obs=t(T + 1, dtype="f64")), dict(obs=t(T + 1, dtype="i32")),
              dict(obs=t(1, T + 1)), dict(obs=t(0)), dict(obs=t(T + 1, nc=True)), dict(H=T + 1), dict(H=-1),
              dict(t0=-1),
              dict(t0=T + 1), dict(t0=4, H=5), *rows, *vec("loglik_in", K), dict(theta=t(K, 3), x_start=t(3)),
              dict(x_start=t(3), obs=t(0)), dict(H=-1, row0=-1))
    c += _ops("sv_smooth", dict(theta=t(K, 4, dtype="i32")), dict(cloud=t(K * N, 1, 4, dtype="i32")), dict(theta=t(K,
              3)),
              dict(theta=t(0, 4)), *[dict(dt=v) for v in (0.0, -1.0, NAN, INF)], dict(theta=t(K, 3), dt=0.0),
              dict(cloud=t(K * N, 4)), dict(cloud=t(K * N, 2, 4)), dict(cloud=t(K * N - 1, 1, 4)),
              dict(cloud=t(K * N, 1, 4, nc=True)), dict(cloud=t(K * 96, 1, 4)), dict(M=32), dict(M=96), dict(M=128),
              dict(theta=t(65536, 4), cloud=t(65536 * N, 1, 1)), dict(obs=t(T + 1, cpu=True)),
              dict(obs=t(T + 1, dtype="i32")), dict(obs=t(1, T + 1)), dict(obs=t(0)), dict(cloud=t(K * N, 1, T + 1)),
              dict(cloud=t(K * N, 1, T), x_next=t(K * M, 1)), dict(cloud=t(K * N, 1, 0)), dict(t0=-1), dict(t0=T - 3),
              dict(t0=2 ** 31 - 4), *rows, *xnext(1), dict(M=32, obs=t(0)), dict(obs=t(0), t0=-1),
              dict(t0=-1, x_next=t(K * M)), dict(dt=0.0, cloud=t(K * N, 2, 4)))
    for fn in ("pmmh", "pmmh_adaptive"):
        c += _ops(fn, dict(theta_cur=t(K, P, dtype="i32")), dict(prior=t(P, 3)), dict(prior=t(P, 2, dtype="i32")),
                  dict(x_start=t(2)), dict(x_start=t(1, 1)), dict(obs=t(1, T, dtype="i32")),
                  dict(obs_bin=t(1, T, dtype="i32")), dict(prior=t(P, 2, cpu=True)), dict(obs=t(1, T, nc=True)),
                  *vec("ll_cur", K), dict(prior=t(P, 3), ll_cur=t(K, dtype="f32")))
    c += _ops("pmmh", dict(prop_chol=t(P, P + 1)), dict(prop_chol=t(K, P, P)), dict(prop_chol=t(P, P, dtype="i32")),
              dict(prop_chol=t(P, P + 1), prior=t(P, 3)))
    c += _ops("pmmh_adaptive", dict(chol_in=t(K, P, P, dtype="i32")), dict(chol_in=t(K, P, P, cpu=True)))
    for fn in ("sv_pmmh", "sv_pmmh_adaptive", "sv_cpmmh"):
        c += _ops(fn, dict(theta_cur=t(K, 4, dtype="i32")), dict(prior=t(4, 3)), dict(prior=t(4, 2, dtype="i32")),
                  dict(h_start=t(2)), dict(h_start=t(1, 1)), dict(obs=t(T + 1, dtype="i32")), dict(obs=t(1, T + 1)),
                  dict(obs=t(0)), dict(prior=t(4, 2, cpu=True)), dict(obs=t(T + 1, nc=True)),
                  *vec("ll_cur", K), dict(prior=t(4, 3), ll_cur=t(K, dtype="f32")), dict(obs=t(1, T + 1), prior=t(4,
                  3)))
    c += _ops("sv_pmmh", dict(prop_chol=t(4, 5)), dict(prop_chol=t(K, 4, 4)), dict(prop_chol=t(4, 4, dtype="i32")))
    for fn in ("sv_pmmh_adaptive", "sv_cpmmh"):
        c += _ops(fn, dict(chol_in=t(K, 4, 4, dtype="i32")), dict(chol_in=t(K, 4, 4, cpu=True)))
    aux = lambda lead: [dict(aux_n=t(*lead, 2, N, 4, cpu=True)), dict(aux_n=t(*lead, 2, N, 4, dtype="f64")),
                        dict(aux_n=t(*lead, 3, N, 4)), dict(aux_n=t(*lead, 2, N, 4, nc=True)), dict(aux_n=t(*lead, 2,
                        N * 4)),
                        dict(aux_r=t(*lead, T, cpu=True)), dict(aux_r=t(*lead, T, dtype="i32")),
                        dict(aux_r=t(*lead, T + 1)), dict(aux_r=t(*lead, T, nc=True)),
                        dict(aux_n=t(*lead, 3, N, 4), aux_r=t(*lead, T + 1))]
    c += _ops("sv_cpmmh", dict(obs=t(1)), dict(chol_in=t(K, 4, 5)), dict(chol_in=t(4, 4)), *aux((K, 2)),
              dict(aux_n=t(K, 2, N, 4)),
              *vec("aux_sel", K, "i32", "i64"), dict(aux_sel=t(K, dtype="i32", fill=2)),
              dict(aux_sel=t(K, dtype="i32", fill=-1)), dict(aux_sel=t(K, dtype="i32", fill=2), aux_r=t(K, 2, T + 1)),
              dict(ll_cur=t(K, dtype="f32"), aux_n=t(K, 2, 3, N, 4)), dict(N=128))
    c += _ops("sv_filter_sorted", dict(theta=t(K, 4, dtype="i32")), dict(x_start=t(1, dtype="i32")), dict(theta=t(K,
              3)),
              dict(theta=t(4)), dict(theta=t(2 ** 21, 4), N=1024), dict(x_start=t(3)),
              dict(x_start=t(K * N + 1)), dict(obs=t(T + 1, dtype="i32")), dict(obs=t(1, T + 1)), dict(obs=t(0)),
              dict(obs=t(1)), dict(obs=t(T + 1, cpu=True)), *aux((K,)), dict(N=128), dict(x_start=t(3), obs=t(1)),
              dict(obs=t(1), aux_n=t(K, 3, N, 4)))
    return c


def record(cases, dev):
    rows = []
    for case in cases:
        e = run_case(case, dev)
        rows.append({**case, "class": type(e).__name__, "message": str(e)})
    return rows


def load_table():
    """The table as {"host": [case], "gpu": [case]}; the file holds a case per line as [fn, kwargs, class, message] (and
    the stub's arguments, for a diagnostics method)."""
    with open(TABLE) as f:
        raw = json.load(f)
    keys = ("fn", "kwargs", "class", "message", "stub")
    return {sec: [dict(zip(keys, row)) for row in rows] for sec, rows in raw.items()}


def dump_table(table, path):
    keys = ("fn", "kwargs", "class", "message")
    row = lambda c: json.dumps([c[k] for k in keys] + ([c["stub"]] if "stub" in c else []), separators=(",", ":"),
                             sort_keys=True)
    sec = lambda name: f' "{name}": [\n  ' + ",\n  ".join(row(c) for c in table[name]) + "\n ]"
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(sec(name) for name in ("host", "gpu")) + "\n}\n")


def case_id(case):
    return case["fn"] + "-" + json.dumps({**case.get("stub", {}), **case["kwargs"]}, separators=(",", ":"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=TABLE)
    args = ap.parse_args()
    table = load_table() if os.path.exists(TABLE) else {"gpu": []}
    table["host"] = record(host_cases(), "cpu")
    if torch.cuda.is_available():
        table["gpu"] = record(gpu_cases(), "cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    dump_table(table, args.out)
    print(f"{args.out}: {len(table['host'])} host cases, {len(table['gpu'])} gpu cases")


if __name__ == "__main__":
    main()
