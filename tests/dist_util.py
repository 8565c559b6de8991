"""Two data-parallel ranks for a test: each rank a fresh child process (spawn) of one gloo group on 127.0.0.1; the GPU
tests' ranks share cuda:0 (RCCL needs one GPU per rank; the 8-GPU run uses RCCL with the same model code).  A test
module gives its own top-level function worker(rank, world, *args) -> payload, which builds the model (attach), makes
the one call under test and returns what the parent compares; run_ranks returns {rank: payload}."""
import os
import queue
import socket
import time

import torch
import torch.multiprocessing as mp


def free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def attach(model, rank: int, world: int, P=None):
    """The model as rank `rank` of `world`: owning samples [rank P / world, (rank + 1) P / world) where P is given."""
    from viforssms_amd.vi_ssm import DistCtx
    model.dist = DistCtx(rank, world)
    if P is not None:
        model.p_local = P // world
    return model


def _rank_main(worker, rank, world, port, out, gpu, args):
    """A rank's process: the group around worker(rank, world, *args), whose payload goes to the parent."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    if gpu:
        torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    payload = worker(rank, world, *args)
    if gpu:
        torch.cuda.synchronize()
    out.put((rank, payload))
    dist.barrier()
    dist.destroy_process_group()


def run_ranks(worker, world: int = 2, timeout: float = 240, gpu: bool = True, args=()):
    """{rank: worker's payload} of `world` ranks.  Fails as soon as a rank has exited with a non-zero code, at the
    deadline, and if a rank does not exit cleanly after reporting: when this returns every child is gone (so the
    parent may touch the GPU)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_rank_main, args=(worker, r, world, port, q, gpu, tuple(args))) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    deadline = time.time() + timeout
    while len(res) < world:
        try:
            rank, payload = q.get(timeout=1)
            res[rank] = payload
        except queue.Empty:
            assert not any(p.exitcode not in (None, 0) for p in procs), "a rank failed"
            assert time.time() < deadline, "timed out"
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res
