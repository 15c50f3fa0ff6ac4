"""The sum of squares of keyed allreduce results on the whole engine at P = 2, 3 over real multi-rank
RCCL on one GPU (the setup of tests/test_multiproc_rccl_gpu.py): one keyed round of mixed requests —
with and without the statistic, uncompressed and over the bf16 wire, one request spanning plans with
plans of its own in the middle (the direct path) — and the data-parallel wrapper's grad_norm, clip and
skip on both of its paths. Every rank checks against the NumPy restatement and against rank 0's bits.
The checks are tests/_mp_sumsq_worker.py's, run by the unchanged _mp_gpu_worker.worker."""
import os
import socket

import pytest

pytestmark = pytest.mark.gpu
CHECKS = ['check_sumsq_keyed_mix', 'check_sumsq_wrapper']


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(world, only, timeout=180.0):
    import torch.multiprocessing as mp

    import _mp_sumsq_worker
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_mp_sumsq_worker.worker, args=(r, world, port, q, only)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(world):
            rank, results = q.get(timeout=float(os.environ.get('DDL_MP_TIMEOUT', timeout)))
            res[rank] = results
    finally:
        for p in procs:
            p.join(timeout=20)
        for p in procs:  # only our own children, by handle
            if p.is_alive():
                p.kill()
                p.join(timeout=10)
    assert sorted(res) == list(range(world)), f'ranks reported: {sorted(res)}'
    for rank, results in sorted(res.items()):
        for name, ok, detail in results:
            assert ok, f'rank {rank} {name}:\n{detail}'
    return res


@pytest.mark.parametrize('world', [2, 3])
def test_sumsq_over_multirank_rccl(gpu, world):
    res = _run(world, CHECKS)
    for rank, results in res.items():
        assert [n for n, _, _ in results] == CHECKS, results
