"""Compression.onebit in the torch mirror, on CPU: the flag reaches the library call for fp32 device tensors only, and
what it cannot carry is a ValueError before any library call."""
import os
import re

import pytest
import torch

from test_wire_mirror_cpu import _Comm, device_kind, recorder  # noqa: F401 (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_reaches_the_engine_and_refusals_come_first(recorder, device_kind, monkeypatch):  # noqa: F811
    from ddl.torch import Compression, cpp_backend as cb, tensor_communicate as tc
    from ddl.torch.compression import wire_flag
    from ddl.torch.parallelism.data import data_parallelism_distributed_optimizer_wrapper as wrap
    with open(os.path.join(ROOT, 'include', 'ddl_amd.h')) as fh:
        assert re.search(r'enum ddl_allreduce_wire_sign \{ DDL_ALLREDUCE_WIRE_SIGN\s*=\s*0x100000\b', fh.read())
    k = Compression.onebit
    assert cb.WIRE_SIGN == wire_flag(k) == 0x100000 and k.feedback and not k.stochastic and repr(k) == 'Compression.onebit'
    with pytest.raises(TypeError, match='onebit'):
        wire_flag('onebit')
    dev32, dev16, host = torch.ones(5), torch.ones(5, dtype=torch.bfloat16), torch.ones(5)
    device_kind += [dev32, dev16]
    sgd = torch.optim.SGD(torch.nn.Linear(3, 2).parameters(), lr=0.1)
    calls = [lambda kw=kw: tc.allreduce_async(dev32, 'a', _Comm(), compression=k, **kw)
             for kw in ({'sumsq': True}, {'op': cb.OP_MIN}, {'op': cb.OP_MAX}, {'op': cb.OP_ADASUM})]
    calls += [lambda kw=kw: wrap(sgd, _Comm(), compression=k, **kw)
              for kw in ({'track_grad_norm': True}, {'max_grad_norm': 1.0}, {'skip_nonfinite': True})]
    for call in calls + [lambda: tc.allreduce_async_batch([dev32], ['a'], _Comm(), compression=k, sumsq=True),
                         lambda: tc.allreduce_gradient(dev32, _Comm(), compression=k)]:
        with pytest.raises(ValueError):
            call()
    assert recorder.calls == []
    for op in (cb.OP_SUM, cb.OP_AVG):
        tc.allreduce_async(dev32, 'a', _Comm(), output=dev32, op=op, compression=k).wait(5)
        assert recorder.calls[-1] == {'keys': ['a'], 'dts': [cb.DT_FLOAT], 'op': op | 0x100000, 'mem': cb.MEMORY_DEVICE}
        for t, mem in ((dev16, cb.MEMORY_DEVICE), (host, cb.MEMORY_HOST)):  # not fp32, not on the device: uncompressed
            tc.allreduce_async(t, 'b', _Comm(), output=t, op=op, compression=k).wait(5)
            assert (recorder.calls[-1]['op'], recorder.calls[-1]['mem']) == (op, mem)
    assert wrap(sgd, _Comm(), compression=k).compression is k
