"""Error feedback of the e4m3 wire on the whole engine in several processes on one GPU: P = 2 and 3 over the test
transport, P = 2 over real multi-rank RCCL (the setup of tests/test_e4m3_multiproc_gpu.py). Two steps of one keyed batch
under stable names (a request cut by sub-plans, factors): the model's bits and the same bytes on every rank; the same
with one rank sending without the bit: other numbers, never a hang. The data-parallel wrapper's check
(check_e4m3_fb_wrapper) is started by tests/test_e4m3_feedback_engine_gpu.py. The checks are
tests/_mp_e4m3_feedback_worker.py's, run by the unchanged _mp_gpu_worker.worker. At most 3 processes hold the GPU at a
time; every child is waited for under a time limit of its own, every exit status is checked, and once a world has
failed no later one is started."""
import os
import queue
import socket
import time

import pytest

pytestmark = pytest.mark.gpu
CHECKS = ['check_e4m3_fb_steps', 'check_e4m3_fb_disagree']
_failed = []  # worlds that failed in this session: nothing more is started on the GPU after one


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(world, only, transport, timeout=180.0):
    import torch.multiprocessing as mp

    import _mp_e4m3_feedback_worker
    assert not _failed, f'not started: {_failed} failed before'
    _failed.append((world, transport))
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_mp_e4m3_feedback_worker.worker, args=(r, world, port, q, only, transport)) for r in range(world)]
    for p in procs:
        p.start()
    deadline = time.monotonic() + float(os.environ.get('DDL_MP_TIMEOUT', timeout))
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
        assert [n for n, _, _ in results] == only, results
    _failed.remove((world, transport))
    return res


@pytest.mark.parametrize('world', [2, 3])
def test_e4m3_feedback_over_test_transport(gpu, world):
    _run(world, CHECKS, 'gloo')


def test_e4m3_feedback_over_multirank_rccl(gpu):
    _run(2, CHECKS, 'rccl')
