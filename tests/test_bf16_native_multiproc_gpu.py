"""The sum of squares and the scale factors of NATIVE bfloat16 keyed allreduces on the whole engine in several
processes on one GPU: P = 2 and 3 over the test transport, P = 2 over real multi-rank RCCL (the setup of
tests/test_multiproc_rccl_gpu.py). A keyed batch mixing bf16 and fp32 requests with and without the options,
SUM and AVG; ranks that pass different postscales; the data-parallel wrapper on a bf16 MLP with
track_grad_norm, max_grad_norm, fused_mean, gradient_predivide_factor, loss_scale and DynamicLossScaler on both
paths, its torch fall-back patched to raise. The checks are tests/_mp_bf16_native_worker.py's, run by the
unchanged _mp_gpu_worker.worker; every process runs under this test's timeout."""
import os
import socket

import pytest

pytestmark = pytest.mark.gpu
KEYED = ['check_bf16_native_keyed_mix']
WRAPPER = ['check_bf16_native_wrapper']


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(world, only, transport, timeout=180.0):
    import torch.multiprocessing as mp

    import _mp_bf16_native_worker
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_mp_bf16_native_worker.worker, args=(r, world, port, q, only, transport)) for r in range(world)]
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
def test_bf16_native_over_test_transport(gpu, world):
    _run(world, KEYED + (WRAPPER if world == 2 else []), 'gloo')


def test_bf16_native_over_multirank_rccl(gpu):
    _run(2, KEYED + WRAPPER, 'rccl')
