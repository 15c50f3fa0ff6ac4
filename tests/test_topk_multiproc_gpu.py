"""DDL_ALLREDUCE_WIRE_TOPK at P = 2 processes over RCCL on one GPU: the check of tests/_mp_topk_worker.py."""
import pytest

import _mp_gpu_worker
import _mp_topk_worker
from test_multiproc_rccl_gpu import _run

pytestmark = pytest.mark.gpu
CHECKS = ['check_topk_batch']


def test_topk_over_multirank_rccl(gpu, monkeypatch):
    monkeypatch.setattr(_mp_gpu_worker, 'worker', _mp_topk_worker.worker)  # what _run spawns, with 'rccl'
    assert all([n for n, _, _ in results] == CHECKS for results in _run(2, CHECKS).values())
