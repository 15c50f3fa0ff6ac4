"""Compression.powersgd in the torch mirror, on CPU: the flag reaches the library call for fp32 device tensors only,
what it cannot carry is a ValueError before any library call, and set_powersgd_rank keeps to 1 .. 16."""
import os
import re

import pytest
import torch

from test_wire_mirror_cpu import _Comm, device_kind, recorder  # noqa: F401 (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_reaches_the_engine_and_refusals_come_first(recorder, device_kind, monkeypatch):  # noqa: F811
    from ddl.torch import Compression, config, cpp_backend as cb, tensor_communicate as tc
    from ddl.torch.compression import set_powersgd_rank, wire_flag
    from ddl.torch.parallelism.data import data_parallelism_distributed_optimizer_wrapper as wrap
    with open(os.path.join(ROOT, 'include', 'ddl_amd.h')) as fh:
        assert re.search(r'enum ddl_allreduce_wire_lowrank \{ DDL_ALLREDUCE_WIRE_LOWRANK\s*=\s*0x200000\b', fh.read())
    k = Compression.powersgd
    assert cb.WIRE_LOWRANK == wire_flag(k) == 0x200000 and k.feedback and not k.stochastic and repr(k) == 'Compression.powersgd'
    assert 'wire_lowrank_rank' in config.KEYS and 'wire_lowrank_rank' in config.SHARED
    with pytest.raises(TypeError, match='powersgd'):
        wire_flag('powersgd')
    dev32, dev16, host = torch.ones(5), torch.ones(5, dtype=torch.bfloat16), torch.ones(5)
    device_kind += [dev32, dev16]
    sgd = torch.optim.SGD(torch.nn.Linear(3, 2).parameters(), lr=0.1)
    calls = [lambda kw=kw: tc.allreduce_async(dev32, 'a', _Comm(), compression=k, **kw)
             for kw in ({'sumsq': True}, {'op': cb.OP_MIN}, {'op': cb.OP_MAX}, {'op': cb.OP_ADASUM})]
    calls += [lambda kw=kw: wrap(sgd, _Comm(), compression=k, **kw)
              for kw in ({'track_grad_norm': True}, {'max_grad_norm': 1.0}, {'skip_nonfinite': True})]
    calls += [lambda v=v: set_powersgd_rank(v) for v in (0, 17, 2.0, True)]
    for call in calls + [lambda: tc.allreduce_async_batch([dev32], ['a'], _Comm(), compression=k, sumsq=True),
                         lambda: tc.allreduce_gradient(dev32, _Comm(), compression=k)]:
        with pytest.raises(ValueError):
            call()
    assert recorder.calls == []
    for op in (cb.OP_SUM, cb.OP_AVG):
        tc.allreduce_async(dev32, 'a', _Comm(), output=dev32, op=op, compression=k).wait(5)
        assert recorder.calls[-1] == {'keys': ['a'], 'dts': [cb.DT_FLOAT], 'op': op | 0x200000, 'mem': cb.MEMORY_DEVICE}
        for t, mem in ((dev16, cb.MEMORY_DEVICE), (host, cb.MEMORY_HOST)):  # not fp32, not on the device: uncompressed
            tc.allreduce_async(t, 'b', _Comm(), output=t, op=op, compression=k).wait(5)
            assert (recorder.calls[-1]['op'], recorder.calls[-1]['mem']) == (op, mem)
    assert wrap(sgd, _Comm(), compression=k).compression is k
