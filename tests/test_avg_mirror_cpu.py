"""The op in the torch mirror, on CPU: allreduce_async_batch hands DDL_ALLREDUCE_OP_AVG to
ddl_allreduce_submit_batch_mem when asked (the default stays SUM), the data-parallel wrapper with
fused_mean submits AVG and never divides, and with the default behaves as before. The engine's side
is a recording submit that completes the slots through ddl_completion_done (as tests/
test_mirror_cpu.py does); every other entry point is the real library's."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Recorder:
    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        return getattr(self._real, name)

    def ddl_get_config(self, key):
        return 0 if key == b'host_register_cache_bytes' else self._real.ddl_get_config(key)

    def ddl_allreduce_submit_batch_mem(self, comm, m, keys, ins, outs, ns, dts, op, mem, stream, done, users):
        self.calls.append({'m': m, 'op': op, 'mem': mem})
        for i in range(m):
            self._real.ddl_completion_done(0, users[i])
        return 0

    def ddl_allreduce_submit_mem(self, comm, key, src, dst, n, dt, op, mem, stream, done, user):
        self.calls.append({'m': 1, 'op': op, 'mem': mem})
        self._real.ddl_completion_done(0, user)
        return 0


class _Comm:
    id, size, rank = 77, 3, 0


@pytest.fixture
def recorder(lib, monkeypatch):
    from ddl.torch.cpp_backend import CPPBackend
    rec = _Recorder(lib)
    monkeypatch.setattr(CPPBackend, 'c_api', staticmethod(lambda: rec))
    return rec


def test_header_declares_avg():
    with open(os.path.join(ROOT, 'include', 'ddl_amd.h')) as f:
        text = f.read()
    assert re.search(r'DDL_ALLREDUCE_OP_SUM\s*=\s*0\s*,\s*DDL_ALLREDUCE_OP_AVG\s*=\s*1\b', text)
    from ddl.torch import cpp_backend as cb
    assert (cb.OP_SUM, cb.OP_AVG) == (0, 1)


def test_batch_submits_the_op(recorder):
    from ddl.torch import cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async, allreduce_async_batch
    ts = [torch.arange(5, dtype=torch.float32), torch.ones(3, dtype=torch.float16)]
    for h in allreduce_async_batch(ts, ['a', 'b'], _Comm(), outputs=ts, op=cb.OP_AVG):
        h.wait(5)
    assert recorder.calls[-1] == {'m': 2, 'op': 1, 'mem': cb.MEMORY_HOST}
    for h in allreduce_async_batch(ts, ['a', 'b'], _Comm(), outputs=ts):
        h.wait(5)
    assert recorder.calls[-1]['op'] == cb.OP_SUM  # the default
    allreduce_async(ts[0], 'c', _Comm(), output=ts[0], op=cb.OP_AVG).wait(5)
    assert recorder.calls[-1]['op'] == cb.OP_AVG
    allreduce_async(ts[0], 'c', _Comm(), output=ts[0]).wait(5)
    assert recorder.calls[-1]['op'] == cb.OP_SUM


def _model_and_wrapper(**kw):
    from ddl.torch.parallelism.data import data_parallelism_distributed_optimizer_wrapper
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Tanh(), torch.nn.Linear(5, 2))
    opt = data_parallelism_distributed_optimizer_wrapper(torch.optim.SGD(model.parameters(), lr=0.1), _Comm(),
                                                         pin_host_gradients=False, **kw)
    return model, opt


def _count_div(monkeypatch):
    calls = []
    real = torch.Tensor.div_

    def counting(self, *a, **k):
        calls.append(a)
        return real(self, *a, **k)
    monkeypatch.setattr(torch.Tensor, 'div_', counting)
    return calls


@pytest.mark.parametrize('overlap', [False, True])
def test_wrapper_fused_mean_submits_avg_and_never_divides(recorder, monkeypatch, overlap):
    from ddl.torch import cpp_backend as cb
    model, opt = _model_and_wrapper(fused_mean=True, overlap_backward=overlap, bucket_bytes=None)
    divs = _count_div(monkeypatch)
    model(torch.randn(4, 6)).sum().backward()
    grads = [p.grad.clone() for p in model.parameters()]
    opt.allreduce_gradients()
    assert sum(c['m'] for c in recorder.calls) == 4 and all(c['op'] == cb.OP_AVG for c in recorder.calls)
    assert not divs
    # the recording engine leaves the gradients alone: nothing here has divided them either
    assert all(torch.equal(p.grad, g) for p, g in zip(model.parameters(), grads))


def test_wrapper_default_sums_and_divides_as_before(recorder, monkeypatch):
    from ddl.torch import cpp_backend as cb
    model, opt = _model_and_wrapper()
    divs = _count_div(monkeypatch)
    model(torch.randn(4, 6)).sum().backward()
    grads = [p.grad.clone() for p in model.parameters()]
    opt.allreduce_gradients()
    assert recorder.calls == [{'m': 4, 'op': cb.OP_SUM, 'mem': cb.MEMORY_HOST}]
    assert [a for a in divs] == [(3,)] * 4
    assert all(torch.equal(p.grad, g / 3) for p, g in zip(model.parameters(), grads))
