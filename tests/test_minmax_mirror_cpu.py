"""MIN / MAX in the torch mirror, on CPU: the constants are the header's, the op reaches the
library call of every allreduce entry point (the recording engine of tests/test_avg_mirror_cpu.py),
a compression with MIN / MAX is a ValueError before any library call, and MetricAverage without
`ops` submits and divides exactly as before."""
import ctypes
import os
import re

import pytest
import torch

from test_avg_mirror_cpu import _Comm, _Recorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _DirectRecorder(_Recorder):
    """Also records the direct collectives (and performs none); a single keyed request completes
    with its input as the result (out = in, a one-rank world's answer)."""

    def ddl_allreduce_submit_mem(self, comm, key, src, dst, n, dt, op, mem, stream, done, user):
        if src != dst:
            ctypes.memmove(dst, src, n * self._real.ddl_dtype_size(dt))
        return super().ddl_allreduce_submit_mem(comm, key, src, dst, n, dt, op, mem, stream, done, user)

    def ddl_allreduce(self, comm, src, dst, n, dt, op, stream):
        self.calls.append({'fn': 'ddl_allreduce', 'op': op})
        return 0

    def ddl_allreduce_host(self, comm, src, dst, n, dt, op):
        self.calls.append({'fn': 'ddl_allreduce_host', 'op': op})
        return 0

    def ddl_allreduce_batch(self, comm, k, ins, outs, ns, dt, op, stream):
        self.calls.append({'fn': 'ddl_allreduce_batch', 'op': op})
        return 0


@pytest.fixture
def recorder(lib, monkeypatch):
    from ddl.torch.cpp_backend import CPPBackend
    rec = _DirectRecorder(lib)
    monkeypatch.setattr(CPPBackend, 'c_api', staticmethod(lambda: rec))
    return rec


def test_constants_match_the_header():
    with open(os.path.join(ROOT, 'include', 'ddl_amd.h')) as f:
        text = f.read()
    m = re.search(r'enum\s+ddl_allreduce_op\s*\{([^}]*)\}', text)
    assert m
    enum = {k: int(v, 0) for k, v in re.findall(r'DDL_ALLREDUCE_OP_(\w+)\s*=\s*(\w+)', m.group(1))}
    assert enum == {'SUM': 0, 'AVG': 1, 'MIN': 3, 'MAX': 4}
    from ddl.torch import cpp_backend as cb
    assert (cb.OP_SUM, cb.OP_AVG, cb.OP_MIN, cb.OP_MAX) == (0, 1, 3, 4)


def test_the_op_reaches_the_library_call(recorder, monkeypatch):
    from ddl.torch import cpp_backend as cb
    from ddl.torch import tensor_communicate as tc
    ts = [torch.arange(5, dtype=torch.float32), torch.ones(3, dtype=torch.int32)]
    for op in (cb.OP_MIN, cb.OP_MAX):
        for h in tc.allreduce_async_batch(ts, ['a', 'b'], _Comm(), outputs=ts, op=op):
            h.wait(5)
        assert recorder.calls[-1] == {'m': 2, 'op': op, 'mem': cb.MEMORY_HOST}
        tc.allreduce_async(ts[0], 'c', _Comm(), output=ts[0], op=op).wait(5)
        assert recorder.calls[-1] == {'m': 1, 'op': op, 'mem': cb.MEMORY_HOST}
        # a CPU tensor: the host pipeline (its pinned output needs a GPU: plain memory here)
        real_empty = torch.empty
        monkeypatch.setattr(torch, 'empty', lambda *a, pin_memory=False, **k: real_empty(*a, **k))
        tc.allreduce(ts[0], _Comm(), op=op)
        assert recorder.calls[-1] == {'fn': 'ddl_allreduce_host', 'op': op}
        # the device entry points, their device checks aside (no GPU here)
        monkeypatch.setattr(tc, 'require_device_tensor', lambda t, what: None)
        monkeypatch.setattr(tc, 'current_stream_handle', lambda device: None)
        tc.allreduce_(ts[0], _Comm(), op=op)
        assert recorder.calls[-1] == {'fn': 'ddl_allreduce', 'op': op}
        tc.allreduce_batch_([ts[0], ts[0].clone()], _Comm(), op=op)
        assert recorder.calls[-1] == {'fn': 'ddl_allreduce_batch', 'op': op}
        monkeypatch.undo()
        monkeypatch.setattr(cb.CPPBackend, 'c_api', staticmethod(lambda: recorder))


def test_compression_with_min_max_is_a_value_error(recorder):
    from ddl.torch import cpp_backend as cb
    from ddl.torch.compression import Compression
    from ddl.torch.tensor_communicate import allreduce_async, allreduce_async_batch
    t = torch.ones(4)
    for op in (cb.OP_MIN, cb.OP_MAX):
        for c in (Compression.fp16, Compression.bf16, Compression.fp16_feedback, Compression.bf16_feedback):
            with pytest.raises(ValueError):
                allreduce_async(t, 'x', _Comm(), op=op, compression=c)
            with pytest.raises(ValueError):
                allreduce_async_batch([t], ['x'], _Comm(), op=op, compression=c)
        assert recorder.calls == []  # refused before any library call
        allreduce_async(t, 'x', _Comm(), op=op, compression=Compression.none).wait(5)
        allreduce_async(t, 'y', _Comm(), op=op, compression=None).wait(5)
        assert [c['op'] for c in recorder.calls] == [op, op]
        recorder.calls.clear()
    allreduce_async(t, 'z', _Comm(), op=cb.OP_AVG, compression=Compression.fp16).wait(5)  # as before: allowed


def test_metric_average_default_is_unchanged_and_ops_are_submitted(recorder):
    from ddl.torch import cpp_backend as cb
    from ddl.torch.parallelism.data import MetricAverage
    logs = {'loss': 6.0, 'acc': 0.75, 'best': 2.0}
    out = MetricAverage(_Comm(), device='cpu').on_epoch_end(0, dict(logs))
    # the recording engine completes every request with the input in place: SUM submitted, divided by 3
    assert [c['op'] for c in recorder.calls] == [cb.OP_SUM] * 3
    assert out == {k: v / 3 for k, v in logs.items()}
    recorder.calls.clear()
    out = MetricAverage(_Comm(), device='cpu', ops={'best': cb.OP_MAX, 'acc': cb.OP_AVG}).on_epoch_end(0, dict(logs))
    assert [c['op'] for c in recorder.calls] == [cb.OP_AVG, cb.OP_MAX, cb.OP_SUM]  # sorted names: acc, best, loss
    assert out == {'loss': 2.0, 'acc': 0.75, 'best': 2.0}  # only the metric without an op is divided here
    with pytest.raises(ValueError):
        MetricAverage(_Comm(), device='cpu', ops={'loss': 2})
