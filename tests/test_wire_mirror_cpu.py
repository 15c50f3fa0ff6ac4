"""Wire compression in the torch mirror, on CPU: the header's flag values and their mirror in
cpp_backend, `compression=` OR-ing the flag into the op of fp32 device-kind requests only, mixed
batches split into a compressed and a plain submission with the handles in the caller's order, and
the data-parallel wrapper (default: plain ops; with compression and fused_mean off it still
divides). The engine's side is a recording submit that completes the slots through
ddl_completion_done (as tests/test_avg_mirror_cpu.py does). There is no device here, so the tensors
that stand for device tensors are CPU tensors whose memory kind the test reports as device."""
import os
import re

import pytest
import torch

from _wire_helpers import WIRE_BF16, WIRE_FP16, test_cpu_reference_values  # noqa: F401 (collected here)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Recorder:
    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        return getattr(self._real, name)

    def ddl_get_config(self, key):
        return 0 if key == b'host_register_cache_bytes' else self._real.ddl_get_config(key)

    def ddl_allreduce_submit_batch_mem(self, comm, m, keys, ins, outs, ns, dts, op, mem, stream, done, users):
        self.calls.append({'keys': [keys[i].decode() for i in range(m)], 'dts': [dts[i] for i in range(m)], 'op': op,
                           'mem': mem})
        for i in range(m):
            self._real.ddl_completion_done(0, users[i])
        return 0

    def ddl_allreduce_submit_mem(self, comm, key, src, dst, n, dt, op, mem, stream, done, user):
        self.calls.append({'keys': [key.decode()], 'dts': [dt], 'op': op, 'mem': mem})
        self._real.ddl_completion_done(0, user)
        return 0


class _Comm:
    id, size, rank = 77, 3, 0


class _Solo:
    id, size, rank = 78, 1, 0


@pytest.fixture
def recorder(lib, monkeypatch):
    from ddl.torch.cpp_backend import CPPBackend
    rec = _Recorder(lib)
    monkeypatch.setattr(CPPBackend, 'c_api', staticmethod(lambda: rec))
    return rec


@pytest.fixture
def device_kind(monkeypatch):
    """Tensors added to the returned list are reported as device memory to tensor_communicate."""
    from ddl.torch import cpp_backend as cb, tensor_communicate as tc
    pretend = []

    def kind(t, what='tensor'):
        return cb.MEMORY_DEVICE if any(t is p for p in pretend) else cb.MEMORY_HOST
    monkeypatch.setattr(tc, 'memory_kind', kind)
    monkeypatch.setattr(tc, 'stream_handle_for', lambda t: 0)
    return pretend


def test_header_declares_the_wire_flags():
    with open(os.path.join(ROOT, 'include', 'ddl_amd.h')) as f:
        text = f.read()
    assert re.search(r'DDL_ALLREDUCE_WIRE_FP16\s*=\s*0x100\s*,\s*DDL_ALLREDUCE_WIRE_BF16\s*=\s*0x200\b', text)
    from ddl.torch import Compression, cpp_backend as cb
    assert (cb.WIRE_FP16, cb.WIRE_BF16) == (0x100, 0x200) == (WIRE_FP16, WIRE_BF16)
    assert (Compression.none.flag, Compression.fp16.flag, Compression.bf16.flag) == (0, 0x100, 0x200)


def test_compression_applies_to_fp32_device_requests_only(recorder, device_kind):
    from ddl.torch import Compression, cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async
    dev32, dev16, host32 = torch.ones(5), torch.ones(5, dtype=torch.float16), torch.ones(5)
    device_kind += [dev32, dev16]
    for comp, flag in ((Compression.fp16, WIRE_FP16), (Compression.bf16, WIRE_BF16)):
        for op in (cb.OP_SUM, cb.OP_AVG):
            allreduce_async(dev32, 'a', _Comm(), output=dev32, op=op, compression=comp).wait(5)
            assert recorder.calls[-1] == {'keys': ['a'], 'dts': [cb.DT_FLOAT], 'op': op | flag, 'mem': cb.MEMORY_DEVICE}
            allreduce_async(dev16, 'b', _Comm(), output=dev16, op=op, compression=comp).wait(5)
            assert recorder.calls[-1]['op'] == op  # not fp32
            allreduce_async(host32, 'c', _Comm(), output=host32, op=op, compression=comp).wait(5)
            assert recorder.calls[-1] == {'keys': ['c'], 'dts': [cb.DT_FLOAT], 'op': op, 'mem': cb.MEMORY_HOST}
    allreduce_async(dev32, 'a', _Comm(), output=dev32).wait(5)
    assert recorder.calls[-1]['op'] == cb.OP_SUM  # the default
    allreduce_async(dev32, 'a', _Comm(), output=dev32, compression=Compression.none).wait(5)
    assert recorder.calls[-1]['op'] == cb.OP_SUM
    allreduce_async(dev32, 'a', _Solo(), output=dev32, compression=Compression.fp16).wait(5)
    assert recorder.calls[-1]['op'] == cb.OP_SUM  # a one-rank world communicates nothing
    with pytest.raises(TypeError):
        allreduce_async(dev32, 'a', _Comm(), output=dev32, compression='fp16')


def test_mixed_batch_is_split_and_keeps_the_handle_order(recorder, device_kind):
    from ddl.torch import Compression, cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async_batch
    ts = [torch.ones(3), torch.ones(4, dtype=torch.float16), torch.ones(5), torch.ones(6), torch.ones(7, dtype=torch.float64)]
    device_kind += [ts[0], ts[1], ts[2], ts[4]]  # ts[3] stays a host tensor
    names = ['k0', 'k1', 'k2', 'k3', 'k4']
    hs = allreduce_async_batch(ts, names, _Comm(), outputs=ts, op=cb.OP_AVG, compression=Compression.bf16)
    assert [h.key for h in hs] == names
    for t, h in zip(ts, hs):
        assert h.wait(5) is t
    assert recorder.calls == [
        {'keys': ['k1', 'k4'], 'dts': [cb.DT_HALF, cb.DT_DOUBLE], 'op': cb.OP_AVG, 'mem': cb.MEMORY_DEVICE},
        {'keys': ['k0', 'k2'], 'dts': [cb.DT_FLOAT, cb.DT_FLOAT], 'op': cb.OP_AVG | WIRE_BF16, 'mem': cb.MEMORY_DEVICE},
        {'keys': ['k3'], 'dts': [cb.DT_FLOAT], 'op': cb.OP_AVG, 'mem': cb.MEMORY_HOST}]
    del recorder.calls[:]
    # without compression the same batch goes as one submission per memory kind, as before
    for h in allreduce_async_batch(ts, names, _Comm(), outputs=ts):
        h.wait(5)
    assert [(c['keys'], c['op']) for c in recorder.calls] == [(['k0', 'k1', 'k2', 'k4'], 0), (['k3'], 0)]
    del recorder.calls[:]
    # an all-fp32 device batch: one compressed submission
    for h in allreduce_async_batch([ts[0], ts[2]], ['k0', 'k2'], _Comm(), compression=Compression.fp16,
                                   outputs=[ts[0], ts[2]]):
        h.wait(5)
    assert [(c['keys'], c['op']) for c in recorder.calls] == [(['k0', 'k2'], WIRE_FP16)]


def _model_and_wrapper(device_kind, **kw):
    from ddl.torch.parallelism.data import data_parallelism_distributed_optimizer_wrapper
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Tanh(), torch.nn.Linear(5, 2))
    opt = data_parallelism_distributed_optimizer_wrapper(torch.optim.SGD(model.parameters(), lr=0.1), _Comm(),
                                                         pin_host_gradients=False, **kw)
    model(torch.randn(4, 6)).sum().backward()
    return model, opt


def _count_div(monkeypatch):
    calls = []
    real = torch.Tensor.div_

    def counting(self, *a, **k):
        calls.append(a)
        return real(self, *a, **k)
    monkeypatch.setattr(torch.Tensor, 'div_', counting)
    return calls


def test_wrapper_default_submits_plain_ops(recorder, device_kind, monkeypatch):
    from ddl.torch import cpp_backend as cb
    model, opt = _model_and_wrapper(device_kind)
    device_kind += [p.grad for p in model.parameters()]
    divs = _count_div(monkeypatch)
    opt.allreduce_gradients()
    assert [(len(c['keys']), c['op']) for c in recorder.calls] == [(4, cb.OP_SUM)]
    assert divs == [(3,)] * 4


@pytest.mark.parametrize('overlap', [False, True])
@pytest.mark.parametrize('fused', [False, True])
def test_wrapper_passes_compression_on_both_paths(recorder, device_kind, monkeypatch, overlap, fused):
    """step() and the overlap_backward hooks submit the flag; with fused_mean off the div_ still
    runs on the fp32 result, with it on AVG | flag is submitted and nothing divides."""
    from ddl.torch import Compression, cpp_backend as cb
    from ddl.torch import tensor_communicate as tc
    if overlap:  # the hooks fire inside backward: every fp32 tensor they submit counts as a device tensor
        monkeypatch.setattr(tc, 'memory_kind', lambda t, what='tensor': cb.MEMORY_DEVICE)
    divs = _count_div(monkeypatch)
    model, opt = _model_and_wrapper(device_kind, compression=Compression.fp16, fused_mean=fused, overlap_backward=overlap,
                                    bucket_bytes=None)
    device_kind += [p.grad for p in model.parameters()]
    grads = [p.grad.clone() for p in model.parameters()]
    opt.allreduce_gradients()
    op = (cb.OP_AVG if fused else cb.OP_SUM) | WIRE_FP16
    assert sum(len(c['keys']) for c in recorder.calls) == 4 and all(c['op'] == op for c in recorder.calls)
    assert [a for a in divs] == ([] if fused else [(3,)] * 4)
    scale = 1 if fused else 3
    assert all(torch.equal(p.grad, g / scale) for p, g in zip(model.parameters(), grads))


@pytest.mark.parametrize('fused', [False, True])
def test_allreduce_gradient_takes_the_keyed_path_when_compressed(recorder, monkeypatch, fused):
    """A dense fp32 device gradient with compression is one keyed request with the flag (the wire
    format belongs to the keyed path); fused_mean picks AVG | flag, otherwise the div_ runs on the
    fp32 result. A CPU gradient is reduced as without compression."""
    from ddl.torch import Compression, cpp_backend as cb
    from ddl.torch import tensor_communicate as tc
    monkeypatch.setattr(tc, 'memory_kind', lambda t, what='tensor': cb.MEMORY_DEVICE)
    monkeypatch.setattr(tc, 'stream_handle_for', lambda t: 0)
    divs = _count_div(monkeypatch)
    g = torch.ones(2, 3)
    out = tc.allreduce_gradient(g, _Comm(), fused_mean=fused, compression=Compression.bf16)
    assert out.shape == g.shape and out.dtype == torch.float32
    assert len(recorder.calls) == 1 and recorder.calls[0]['dts'] == [cb.DT_FLOAT]
    assert recorder.calls[0]['op'] == (cb.OP_AVG if fused else cb.OP_SUM) | WIRE_BF16
    assert divs == ([] if fused else [(3,)])
    tc.allreduce_gradient(g, _Comm(), fused_mean=fused, compression=Compression.bf16)
    assert recorder.calls[1]['keys'] != recorder.calls[0]['keys']  # a running name per request
