"""Draw seeds of tests/test_gpu_stage_ahead.py, chosen on the CPU from the rounding model alone (the rule documented in
tests/test_gpu_bwd2_ahead.py): per shape, the first seed from 18 upwards whose four-realisation ELBO envelope (the
maximum over the EMUL_REALISATIONS realisations the test's bar is built from) is not below the rms of the same figure
over 24 realisations of the model.  Also asserts what the test asserts of the reference: finite oracle ELBOs and no
exactly-zero oracle gradient.  No GPU: the model is built on the CPU and only the float64 oracle runs.

usage: python scripts/stage_ahead_draws.py [shape ...]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from oracle.precision_model import PRECISION_MODE, emulate
from tests.parity_util import EMUL_REALISATIONS, build_model, oracle_reference
from tests.test_gpu_stage_ahead import MODEL_SEED, SHAPES
from viforssms_amd._lib import TRAIN_PRECISIONS as PREC

N_RMS = 24


def main():
    for shape in sys.argv[1:] or list(SHAPES):
        B, M, k, H, _ = SHAPES[shape]
        model = build_model("ar", B, M, k, 3, H, 3, 3, "cpu", precision=PREC["bf16"], seed=MODEL_SEED)
        md, st = model.mdef, model.store
        batch = model.engine.make_batch(np.zeros(B, dtype=np.int64))
        for seed in range(18, 40):
            g = torch.Generator().manual_seed(seed)
            eps = torch.randn(B, md.kernel_ext, generator=g, dtype=torch.float64)
            x0 = torch.randn(B, md.P_theta, generator=g, dtype=torch.float64) * md.theta_base[1] + md.theta_base[0]
            elbo_ref, ref_g = oracle_reference(model, batch, eps, x0)
            ok = bool(np.isfinite(elbo_ref).all()) and all(np.linalg.norm(ref_g[n]) > 0 for n in st.names())
            errs = []
            for r in range(N_RMS):
                with emulate(PRECISION_MODE[PREC["bf16"]], realisation=r):
                    e_em, _ = oracle_reference(model, batch, eps, x0)
                errs.append(float(np.max(np.abs(e_em - elbo_ref) / np.maximum(np.abs(elbo_ref), 1e-6))))
            env, rms = max(errs[:EMUL_REALISATIONS]), float(np.sqrt(np.mean(np.square(errs))))
            take = ok and env >= rms
            print(f"{shape:12s} seed {seed}: envelope of {EMUL_REALISATIONS} {env:.3e}, rms of {N_RMS} {rms:.3e}, "
                  f"max {max(errs):.3e}, reference {'ok' if ok else 'NOT usable'} -> {'taken' if take else 'next'}",
                  flush=True)
            if take:
                break


if __name__ == "__main__":
    main()
