"""The e4m3 wire over bfloat16 tensors on the whole engine in several processes on one GPU: P = 2 and 3 over the test
transport, P = 2 over multi-rank RCCL. The checks are tests/_mp_e4m3_bf16_worker.py's; the processes are started,
waited for and checked by tests/test_e4m3_multiproc_gpu.py's _run."""
import pytest

import _mp_e4m3_bf16_worker
import _mp_e4m3_worker
from test_e4m3_multiproc_gpu import _run

pytestmark = pytest.mark.gpu
CHECKS = ['check_e4m3_bf16_mixed_batch', 'check_e4m3_bf16_wrapper']


@pytest.mark.parametrize('world,transport', [(2, 'gloo'), (3, 'gloo'), (2, 'rccl')])
def test_e4m3_bf16_multiproc(gpu, monkeypatch, world, transport):
    # _run starts whatever _mp_e4m3_worker.worker names; a spawned child unpickles the function by its own module
    monkeypatch.setattr(_mp_e4m3_worker, 'worker', _mp_e4m3_bf16_worker.worker)
    _run(world, CHECKS, transport)
