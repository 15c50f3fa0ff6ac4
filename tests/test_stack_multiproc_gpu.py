"""The keyed allreduce's options together on the whole engine in several processes on one GPU: P = 2 and 3
over the test transport, P = 2 over real multi-rank RCCL (the setup of tests/test_multiproc_rccl_gpu.py).
A feedback request that spans three fusion plans next to scaled, plain-wire and uncompressed requests
with a sum of squares, three rounds under stable keys; the data-parallel wrapper with bf16 feedback,
fused_mean, gradient_predivide_factor, DynamicLossScaler and track_grad_norm over four steps, one of them
skipped, on the step() path and the overlap_backward hooks. The checks are tests/_mp_stack_worker.py's,
run by the unchanged _mp_gpu_worker.worker; every process runs under this test's timeout."""
import os
import socket

import pytest

pytestmark = pytest.mark.gpu
KEYED = ['check_stack_keyed']
WRAPPER = ['check_stack_wrapper']


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(world, only, transport, timeout=180.0):
    import torch.multiprocessing as mp

    import _mp_stack_worker
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_mp_stack_worker.worker, args=(r, world, port, q, only, transport)) for r in range(world)]
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
        assert [n for n, _, _ in results] == only, results
    return res


@pytest.mark.parametrize('world', [2, 3])
def test_stack_over_test_transport(gpu, world):
    _run(world, KEYED + WRAPPER, 'gloo')


def test_stack_over_multirank_rccl(gpu):
    _run(2, KEYED + WRAPPER, 'rccl')
