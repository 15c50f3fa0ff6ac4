"""DDL_ALLREDUCE_OP_ADASUM at P = 2, 3 processes over RCCL on one GPU: the checks of tests/_mp_adasum_worker.py."""
import pytest

import _mp_adasum_worker
import _mp_gpu_worker
from test_multiproc_rccl_gpu import _run

pytestmark = pytest.mark.gpu
CHECKS = ['check_adasum_batch', 'check_adasum_optimizer']


@pytest.mark.parametrize('world', [2, 3])
def test_adasum_over_multirank_rccl(gpu, world, monkeypatch):
    monkeypatch.setattr(_mp_gpu_worker, 'worker', _mp_adasum_worker.worker)  # what _run spawns, with 'rccl'
    assert all([n for n, _, _ in results] == CHECKS for results in _run(world, CHECKS).values())
