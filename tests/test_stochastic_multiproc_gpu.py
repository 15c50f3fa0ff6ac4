"""Stochastic rounding of the bf16 wire on the whole engine at P = 2, 3 over real multi-rank RCCL on one
GPU (the setup of tests/test_multiproc_rccl_gpu.py): two steps of a keyed batch under the same names (fp32
device tensors of 5, 513 and 70_001 elements with Compression.bf16_stochastic, one native fp16 tensor among
them), then one step() of the data-parallel wrapper with Compression.bf16_stochastic and fused_mean. The
checks are tests/_mp_stochastic_worker.py's, run by the unchanged _mp_gpu_worker.worker. At most 3 processes
hold the GPU at a time; every child is waited for under a time limit of its own, every exit status is
checked, and once a world has failed the later one is not started."""
import os
import socket
import time

import pytest

pytestmark = pytest.mark.gpu
CHECKS = ['check_stochastic_keyed_batch', 'check_stochastic_dp_wrapper']
_failed = []  # worlds that failed in this session: nothing more is started on the GPU after one


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(world, only, timeout=180.0):
    import queue

    import torch.multiprocessing as mp

    import _mp_stochastic_worker
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_mp_stochastic_worker.worker, args=(r, world, port, q, only)) for r in range(world)]
    for p in procs:
        p.start()
    limit = float(os.environ.get('DDL_MP_TIMEOUT', timeout))
    deadline = time.monotonic() + limit
    res = {}
    try:
        while len(res) < world and time.monotonic() < deadline:
            try:
                rank, results = q.get(timeout=1.0)
                res[rank] = results
            except queue.Empty:
                if any(p.exitcode not in (None, 0) for p in procs):
                    break  # a child died: the others would wait for it in vain
    finally:
        for p in procs:  # each child under its own limit; only our own children, by handle
            p.join(timeout=max(1.0, min(20.0, deadline + 20.0 - time.monotonic())))
            if p.is_alive():
                p.kill()
                p.join(timeout=10)
    codes = [p.exitcode for p in procs]
    assert codes == [0] * world, f'exit statuses of the ranks: {codes}; reported: {res}'
    assert sorted(res) == list(range(world)), f'ranks reported: {sorted(res)}'
    for rank, results in sorted(res.items()):
        for name, ok, detail in results:
            assert ok, f'rank {rank} {name}:\n{detail}'
    return res


@pytest.mark.parametrize('world', [2, 3])
def test_stochastic_over_multirank_rccl(gpu, world):
    assert not _failed, f'not started: the world of {_failed} ranks failed before'
    _failed.append(world)
    res = _run(world, CHECKS)
    for rank, results in res.items():
        assert [n for n, _, _ in results] == CHECKS, results
    _failed.remove(world)
