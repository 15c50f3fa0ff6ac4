"""Worker of tests/test_adasum_multiproc_gpu.py: _mp_gpu_worker.worker with these checks added inside the child."""
import numpy as np

import _mp_gpu_worker
from _adasum_helpers import max_excess, tree
from _mp_minmax_worker import _same_as_rank0


def check_adasum_batch(ctx):
    """An Adasum batch of three tensors (one of three tiles) beside a SUM batch of the same dtype in one round."""
    torch, comm, P, r = ctx['torch'], ctx['comm'], ctx['P'], ctx['rank']
    from ddl.torch import cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async_batch
    rng = [np.random.default_rng(40 + q) for q in range(P)]
    xs = [[g.standard_normal(n).astype(np.float32) for n in (5, 4099, 300)] for g in rng]
    ks = [[g.integers(-8, 9, n).astype(np.float32) for n in (5, 4099, 300)] for g in rng]
    ada = allreduce_async_batch([torch.from_numpy(x).cuda() for x in xs[r]], ['ada0', 'ada1', 'ada2'], comm, op=cb.OP_ADASUM)
    plain = allreduce_async_batch([torch.from_numpy(x).cuda() for x in ks[r]], ['sum0', 'sum1', 'sum2'], comm)
    got, sums = [h.wait(timeout=120) for h in ada], [h.wait(timeout=120).cpu().numpy() for h in plain]
    assert all(max_excess(got[i].cpu().numpy(), tree([x[i] for x in xs])) <= 0.0 for i in range(3))
    assert all(np.array_equal(sums[i], np.sum([k[i] for k in ks], axis=0)) for i in range(3))
    _same_as_rank0(ctx, got, 'adasum batch')


def check_adasum_optimizer(ctx):
    """One wrapper step with adasum=True on the 6-5-2 Sequential, gradients from the seeds: the tree, undivided."""
    torch, comm, P, r = ctx['torch'], ctx['comm'], ctx['P'], ctx['rank']
    from ddl.torch.parallelism.data import data_parallelism_distributed_optimizer_wrapper
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Tanh(), torch.nn.Linear(5, 2)).cuda()
    params = list(model.parameters())
    before = [p.detach().clone() for p in params]
    grads = [[np.random.default_rng(70 + 10 * q + i).standard_normal(p.numel()).astype(np.float32)
              for i, p in enumerate(params)] for q in range(P)]
    for p, g in zip(params, grads[r]):
        p.grad = torch.from_numpy(g).cuda().view_as(p)
    data_parallelism_distributed_optimizer_wrapper(torch.optim.SGD(params, lr=0.5), comm, adasum=True).step()
    for i, (p, p0) in enumerate(zip(params, before)):
        assert max_excess(p.grad.cpu().numpy().ravel(), tree([g[i] for g in grads])) <= 0.0, i
        assert torch.equal(p.detach(), p0 - 0.5 * p.grad)
    _same_as_rank0(ctx, [p.grad for p in params], 'adasum optimizer')


def worker(rank, world, port, q, only, transport):
    _mp_gpu_worker.FAULT_CHECKS.update({f.__name__: f for f in (check_adasum_batch, check_adasum_optimizer)})
    _mp_gpu_worker.worker(rank, world, port, q, only=only, transport=transport)
