"""particle_filter(proposal="adapted") over data-parallel ranks (modelled on tests/test_gpu_particle_dist.py): 2 ranks share cuda:0 over gloo (spawned as in
tests/test_gpu_forecast_dist.py; each rank a fresh child process).  theta is rank 0's first rows of the first
window's draw -- the global samples 0 .. K - 1 -- broadcast; every rank then runs the identical deterministic launches,
so both hold, bit for bit, the result of one process holding the full batch."""
import os
import queue
import socket
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

P = 16
SHAPE, T = (P, 30, 5, 2, 20, 3, 4), 60     # AR: (B, M, k, n_flows, H, n_layers, fw), two windows
KF, NF, CHUNK = 6, 128, 25                  # K <= p_local = 8; three launches per rank
KEYS = ("probs", "filter/loglik", "filter/theta", "filter/ll_inc", "filter/ess", "filter/mean", "filter/sd",
        "filter/n_valid", "filter/quantiles", "filter/proposal")


def _eq(a, b):
    """array_equal with NaN == NaN for the float entries (the proposal's name is a string array)."""
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _model():
    from tests.parity_util import build_model
    from tests.sim_util import AR, TRUE_THETA
    model = build_model("ar", *SHAPE, "cuda:0", T=T, precision=0, seed=3)
    # q(theta) at the generator's parameters (tests/test_gpu_particle.py): a random theta_1 above 1 leaves no weight
    vals = model.store.state_numpy()
    name = f"theta/maf{model.mdef.n_maf - 1}/dense3/bias"
    bias = vals[name].copy()
    bias[0::2] = -np.exp(3.0) * np.asarray(TRUE_THETA[AR])
    bias[1::2] = 3.0
    vals[name] = bias
    model.store.load_numpy(vals)
    return model


def _worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from viforssms_amd.vi_ssm import DistCtx
    model = _model()
    model.dist = DistCtx(rank, world)
    model.p_local = P // world
    res = model.particle_filter(KF, NF, chunk=CHUNK, proposal="adapted")
    torch.cuda.synchronize()
    out.put((rank, {k: res[k] for k in KEYS}))
    dist.barrier()
    dist.destroy_process_group()


def _run():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    deadline = time.time() + 240
    while len(res) < 2:
        try:
            r = q.get(timeout=1)
            res[r[0]] = r[1]
        except queue.Empty:
            assert not any(p.exitcode not in (None, 0) for p in procs), "a rank failed"
            assert time.time() < deadline, "timed out"
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


def test_two_rank_adapted_filter_equals_single_process():
    res = _run()      # both children have exited (exit codes checked) before this process touches the GPU
    full = _model().particle_filter(KF, NF, proposal="adapted")
    assert sorted(full) == sorted(KEYS) and np.isfinite(full["filter/loglik"]).any()
    assert str(full["filter/proposal"]) == "adapted"
    assert full["filter/ll_inc"].shape == (KF, T) and full["filter/quantiles"].shape == (5, 1, T)
    for k in KEYS:
        assert _eq(res[0][k], res[1][k]), k
        assert _eq(res[0][k], full[k]), k
