"""Worker of tests/test_topk_multiproc_gpu.py: _mp_gpu_worker.worker with this check added inside the child."""
import numpy as np

import _mp_gpu_worker
from _mp_minmax_worker import _same_as_rank0
from _topk_helpers import AVG, reference


def check_topk_batch(ctx):
    """Two steps of a Compression.topk AVG batch under stable names beside a SUM batch: the numpy rule bit for bit."""
    torch, comm, P, r = ctx['torch'], ctx['comm'], ctx['P'], ctx['rank']
    from ddl.torch import Compression, cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async_batch
    sizes, names = (5, 4099, 300), ['topk0', 'topk1', 'topk2']
    res = [[np.zeros(n, np.float32) for n in sizes] for _ in range(P)]
    for step in range(2):
        xs = [[np.random.default_rng(100 * step + 10 * q + i).standard_normal(n).astype(np.float32)
               for i, n in enumerate(sizes)] for q in range(P)]
        ks = [np.random.default_rng(90 + q).integers(-8, 9, 300).astype(np.float32) for q in range(P)]
        sparse = allreduce_async_batch([torch.from_numpy(x).cuda() for x in xs[r]], names, comm, op=cb.OP_AVG,
                                       compression=Compression.topk)
        plain = allreduce_async_batch([torch.from_numpy(ks[r]).cuda()], ['sum0'], comm)
        got = [h.wait(timeout=120) for h in sparse]
        assert np.array_equal(plain[0].wait(timeout=120).cpu().numpy(), np.sum(ks, axis=0))
        for i in range(3):
            want, new = reference([x[i] for x in xs], [row[i] for row in res], 10_000, AVG)
            for q in range(P):
                res[q][i] = new[q]
            assert got[i].cpu().numpy().tobytes() == want.tobytes(), (step, i)
        _same_as_rank0(ctx, got, 'topk batch')


def worker(rank, world, port, q, only, transport):
    _mp_gpu_worker.FAULT_CHECKS.update({f.__name__: f for f in (check_topk_batch,)})
    _mp_gpu_worker.worker(rank, world, port, q, only=only, transport=transport)
