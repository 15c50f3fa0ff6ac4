"""Compression.topk in the torch mirror, on CPU: the flag reaches the library call, what it cannot carry is a
ValueError before any library call, the density is a shared tunable."""
import os
import re

import pytest
import torch

from test_wire_mirror_cpu import _Comm, device_kind, recorder  # noqa: F401 (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_reaches_the_engine_and_refusals_come_first(recorder, device_kind, monkeypatch):  # noqa: F811
    from ddl.torch import Compression, config, cpp_backend as cb, tensor_communicate as tc
    from ddl.torch.compression import set_topk_density, wire_flag
    from ddl.torch.parallelism.data import data_parallelism_distributed_optimizer_wrapper as wrap
    with open(os.path.join(ROOT, 'include', 'ddl_amd.h')) as fh:
        assert re.search(r'DDL_ALLREDUCE_WIRE_TOPK\s*=\s*0x80000\b', fh.read())
    k = Compression.topk
    assert cb.WIRE_TOPK == wire_flag(k) == 0x80000 and k.feedback and not k.stochastic and repr(k) == 'Compression.topk'
    assert 'wire_topk_ppm' in config.KEYS and 'wire_topk_ppm' in config.SHARED
    dev32, dev16 = torch.ones(5), torch.ones(5, dtype=torch.bfloat16)
    device_kind += [dev32, dev16]
    model = torch.nn.Linear(3, 2)
    for call in (lambda: tc.allreduce_async(dev32, 'a', _Comm(), compression=k, sumsq=True),
                 lambda: tc.allreduce_async_batch([dev32], ['a'], _Comm(), compression=k, sumsq=True),
                 lambda: tc.allreduce_async(dev32, 'a', _Comm(), op=cb.OP_MAX, compression=k),
                 lambda: tc.allreduce_async(dev32, 'a', _Comm(), op=cb.OP_ADASUM, compression=k),
                 lambda: tc.allreduce_gradient(dev32, _Comm(), compression=k),
                 lambda: wrap(torch.optim.SGD(model.parameters(), lr=0.1), _Comm(), compression=k, track_grad_norm=True),
                 lambda: wrap(torch.optim.SGD(model.parameters(), lr=0.1), _Comm(), compression=k, max_grad_norm=1.0),
                 lambda: wrap(torch.optim.SGD(model.parameters(), lr=0.1), _Comm(), compression=k, skip_nonfinite=True),
                 lambda: set_topk_density(2.0)):
        with pytest.raises(ValueError):
            call()
    assert recorder.calls == []
    for op in (cb.OP_SUM, cb.OP_AVG):
        tc.allreduce_async(dev32, 'a', _Comm(), output=dev32, op=op, compression=k).wait(5)
        assert recorder.calls[-1] == {'keys': ['a'], 'dts': [cb.DT_FLOAT], 'op': op | 0x80000, 'mem': cb.MEMORY_DEVICE}
        tc.allreduce_async(dev16, 'b', _Comm(), output=dev16, op=op, compression=k).wait(5)
        assert recorder.calls[-1]['op'] == op  # not fp32: submitted uncompressed
    assert wrap(torch.optim.SGD(model.parameters(), lr=0.1), _Comm(), compression=k).compression is k
