"""OP_ADASUM in the torch mirror, on CPU: what the op cannot carry is a ValueError before any library call."""
import pytest
import torch

from test_avg_mirror_cpu import _Comm, _Recorder


def test_value_errors_before_any_library_call(lib, monkeypatch):
    from ddl.torch import Compression, cpp_backend as cb, tensor_communicate as tc
    from ddl.torch.parallelism.data import data_parallelism_distributed_optimizer_wrapper as wrap
    rec = _Recorder(lib)
    monkeypatch.setattr(cb.CPPBackend, 'c_api', staticmethod(lambda: rec))
    assert cb.OP_ADASUM == 6
    t, model = torch.ones(4), torch.nn.Linear(3, 2)
    for kw in (dict(compression=Compression.fp16), dict(sumsq=True), dict(), dict(tensor=t.to_sparse())):
        x = kw.pop('tensor', t)
        for call in (lambda: tc.allreduce_async(x, 'x', _Comm(), op=cb.OP_ADASUM, **kw),
                     lambda: tc.allreduce_async_batch([x], ['x'], _Comm(), op=cb.OP_ADASUM, **kw),
                     lambda: tc.allreduce_gradient(x, _Comm(), op=cb.OP_ADASUM)):
            with pytest.raises(ValueError):
                call()
    for kw in (dict(fused_mean=True), dict(compression=Compression.bf16), dict(track_grad_norm=True),
               dict(max_grad_norm=1.0), dict(skip_nonfinite=True)):
        with pytest.raises(ValueError):
            wrap(torch.optim.SGD(model.parameters(), lr=0.1), _Comm(), adasum=True, **kw)
    opt = wrap(torch.optim.SGD(model.parameters(), lr=0.1), _Comm(), pin_host_gradients=False, adasum=True)
    assert opt._op() == cb.OP_ADASUM
    model(torch.randn(4, 3)).sum().backward()
    with pytest.raises(ValueError):  # a CPU gradient, at the first step: never a silent mean
        opt.step()
    assert rec.calls == []
