"""Data-parallel path on CPU (gloo, world_size 2): every rank draws the same window starts,
owns samples [r*p_local, (r+1)*p_local), and the SUM all-reduce of the per-rank gradients of
sum(-ELBO) equals the full-batch gradient (the reference's single-process step, AR.py:228-234).
The per-rank gradients come from the oracle (the GPU kernels are covered by tests/test_gpu_parity.py);
what is tested here is the sharding, the window agreement and the collective."""
import numpy as np
import pytest
import torch
import torch.distributed as dist

from oracle import nma_oracle as O
from oracle import bridge
from tests.dist_util import attach, run_ranks

P, M, T, SEED = 4, 50, 300, 5


def _model():
    from tests.parity_util import build_model
    return build_model("ar", P, M, 6, 2, 12, 3, 3, "cpu", T=T, seed=3)


def _oracle_grad(model, starts, rows):
    md = model.mdef
    g = torch.Generator().manual_seed(11)
    eps = torch.randn(P, md.kernel_ext, generator=g, dtype=torch.float64)[rows]
    x0 = (torch.randn(P, md.P_theta, generator=g, dtype=torch.float64) * md.theta_base[1] + md.theta_base[0])[rows]
    batch = model.engine.make_batch(np.asarray(starts)[rows])
    inv = np.unique(np.asarray(starts)[rows], return_inverse=True)[1]
    ts = torch.tensor(batch.ts.double().numpy()[inv], dtype=O.DT)
    spec = bridge.spec_from_mdef(md, len(rows))
    params = bridge.oracle_params(model.store.state_numpy(), spec, model.engine.theta_dist.masks_np)
    leaves = O.param_leaves(params)
    for t in leaves:
        t.requires_grad_(True)
    out = O.elbo(spec, params, model.engine.perms, x0, eps, ts, {})
    grads = torch.autograd.grad((-out["elbo"]).sum(), leaves, allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for t, g in zip(leaves, grads)]
    byname = bridge.oracle_grads_by_name(params, grads, spec)
    return np.concatenate([byname[n].ravel() for n in model.store.names()])


def _worker(rank, world):
    model = attach(_model(), rank, world, P)
    np.random.seed(SEED)
    starts = model.select_windows()
    # every rank must draw the same global window starts
    gathered = [torch.zeros(P, dtype=torch.int64) for _ in range(world)]
    dist.all_gather(gathered, torch.as_tensor(starts))
    same = all(torch.equal(gathered[0], x) for x in gathered)
    local = model.batch_for(starts)
    rows = np.arange(rank * model.p_local, (rank + 1) * model.p_local)
    assert np.array_equal(local.starts, starts[rows])
    grad = torch.tensor(_oracle_grad(model, starts, rows))
    model.dist.all_reduce_(grad)
    return same, starts, grad.numpy()


def test_two_rank_gradient_equals_full_batch():
    same, starts, reduced = run_ranks(_worker, gpu=False)[0]
    assert same
    full = _oracle_grad(_model(), starts, np.arange(P))
    assert np.allclose(reduced, full, rtol=1e-10, atol=1e-10 * np.abs(full).max())


def _overlap_worker(rank, world):
    model = _model()
    model.build_flow()
    attach(model, rank, world)
    st = model.store
    buckets = model._grad_buckets()
    res = []
    for overlap in (True, False):
        model.overlap_allreduce = overlap
        st.zero_grad()
        g = torch.Generator().manual_seed(100 + rank)
        # a loss touching every variable, differently per rank; flows' terms enter in reverse order
        loss = sum((st[n] * torch.randn(st[n].shape, generator=g, dtype=st[n].dtype)).sum() for n in st.names())
        model._arm_overlap()
        loss.backward()
        launched = len(model._ov["handles"]) if model._ov is not None else 0
        model._reduce_grads()
        res.append((launched, st.grad.clone().numpy()))
    return [b[0] for b in buckets], res


def test_bucketed_overlapped_allreduce_equals_blocking_allreduce():
    """The per-flow gradient buckets (launched asynchronously from the accumulate hooks during the
    backward) reduce to exactly the single blocking all-reduce of the flat gradient, on 2 gloo ranks."""
    keys, res = run_ranks(_overlap_worker, gpu=False)[0]
    assert keys == ["flow1", "flow0", "rest"]       # backward completion order, q(theta) last
    (n_ov, g_ov), (n_blk, g_blk) = res
    assert n_ov == 2 and n_blk == 0                 # both flow buckets went out during the backward
    assert np.array_equal(g_ov, g_blk)
