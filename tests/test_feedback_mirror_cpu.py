"""Error feedback of the 16-bit wire in the torch mirror, on CPU: the header's enum line, the
constants and the `Compression` flags, `wire_flag`, the flags reaching the engine's submit entry
points unchanged (and only for fp32 device-kind tensors), allreduce_gradient's ValueError, and
reset_error_feedback moving the engine's `wire_feedback_epoch`. The CPU model's pinned values
(_feedback_helpers.test_cpu_model_values) are collected here too. The recording submit is
tests/test_wire_mirror_cpu.py's."""
import os
import re

import pytest
import torch

from _feedback_helpers import WIRE_FEEDBACK, test_cpu_model_values  # noqa: F401 (collected here)
from _wire_helpers import WIRE_BF16, WIRE_FP16
from test_wire_mirror_cpu import _Comm, _Solo, device_kind, recorder  # noqa: F401 (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_feedback_bit():
    with open(os.path.join(ROOT, 'include', 'ddl_amd.h')) as f:
        text = f.read()
    m = re.search(r'enum\s+ddl_allreduce_wire\s*\{(.*?)\};', text, re.S)
    assert m, 'enum ddl_allreduce_wire'
    body = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)
    names = re.findall(r'(DDL_ALLREDUCE_WIRE_\w+)\s*=\s*(0x[0-9a-fA-F]+)', body)
    assert names == [('DDL_ALLREDUCE_WIRE_FP16', '0x100'), ('DDL_ALLREDUCE_WIRE_BF16', '0x200'),
                     ('DDL_ALLREDUCE_WIRE_FEEDBACK', '0x1000')]
    # the deployment header's function list is unchanged: the feature is an op bit
    assert 'feedback' not in ' '.join(re.findall(r'\b(ddl_\w+)\s*\(', text)).lower()


def test_constants_and_compression_flags():
    from ddl.torch import Compression, cpp_backend as cb
    from ddl.torch.compression import wire_flag
    assert cb.WIRE_FEEDBACK == 0x1000 == WIRE_FEEDBACK
    assert (cb.WIRE_FP16, cb.WIRE_BF16) == (WIRE_FP16, WIRE_BF16)
    assert (Compression.none.flag, Compression.fp16.flag, Compression.bf16.flag) == (0, 0x100, 0x200)
    assert (Compression.fp16_feedback.flag, Compression.bf16_feedback.flag) == (0x1100, 0x1200)
    assert [wire_flag(c) for c in (None, Compression.none, Compression.fp16, Compression.bf16,
                                   Compression.fp16_feedback, Compression.bf16_feedback)] == \
        [0, 0, 0x100, 0x200, 0x1100, 0x1200]
    assert repr(Compression.bf16_feedback) == 'Compression.bf16_feedback'
    for bad in ('bf16_feedback', 0x1200, True):
        with pytest.raises(TypeError):
            wire_flag(bad)
    assert not any('feedback' in n.lower() for n in cb.DEPLOYMENT_API)


def test_docstrings_name_the_cost_and_the_reset():
    import ddl.torch.compression as comp
    from ddl.torch.parallelism.data import distributed_optimizer as do
    for doc in (comp.__doc__, do.__doc__):
        assert '14' in doc and 'fp32 copy' in doc and 'checkpoint' in doc and 'loss scale' in doc
    assert 'checkpoint' in comp.reset_error_feedback.__doc__ and 'loss scale' in comp.reset_error_feedback.__doc__


def test_feedback_flags_reach_the_engine_for_fp32_device_requests_only(recorder, device_kind):  # noqa: F811
    from ddl.torch import Compression, cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async, allreduce_async_batch
    dev32, dev16, host32 = torch.ones(5), torch.ones(5, dtype=torch.float16), torch.ones(5)
    device_kind += [dev32, dev16]
    for comp, flag in ((Compression.fp16_feedback, 0x1100), (Compression.bf16_feedback, 0x1200)):
        for op in (cb.OP_SUM, cb.OP_AVG):
            allreduce_async(dev32, 'a', _Comm(), output=dev32, op=op, compression=comp).wait(5)
            assert recorder.calls[-1] == {'keys': ['a'], 'dts': [cb.DT_FLOAT], 'op': op | flag, 'mem': cb.MEMORY_DEVICE}
            allreduce_async(dev16, 'b', _Comm(), output=dev16, op=op, compression=comp).wait(5)
            assert recorder.calls[-1]['op'] == op  # not fp32: no wire bits at all
            allreduce_async(host32, 'c', _Comm(), output=host32, op=op, compression=comp).wait(5)
            assert recorder.calls[-1] == {'keys': ['c'], 'dts': [cb.DT_FLOAT], 'op': op, 'mem': cb.MEMORY_HOST}
    allreduce_async(dev32, 'a', _Solo(), output=dev32, compression=Compression.bf16_feedback).wait(5)
    assert recorder.calls[-1]['op'] == cb.OP_SUM  # size 1 with the shortcut: nothing is communicated
    del recorder.calls[:]
    ts = [dev32, dev16, host32]
    for h in allreduce_async_batch(ts, ['k0', 'k1', 'k2'], _Comm(), outputs=ts, op=cb.OP_AVG,
                                   compression=Compression.bf16_feedback):
        h.wait(5)
    assert recorder.calls == [
        {'keys': ['k1'], 'dts': [cb.DT_HALF], 'op': cb.OP_AVG, 'mem': cb.MEMORY_DEVICE},
        {'keys': ['k0'], 'dts': [cb.DT_FLOAT], 'op': cb.OP_AVG | 0x1200, 'mem': cb.MEMORY_DEVICE},
        {'keys': ['k2'], 'dts': [cb.DT_FLOAT], 'op': cb.OP_AVG, 'mem': cb.MEMORY_HOST}]


@pytest.mark.parametrize('overlap', [False, True])
def test_wrapper_carries_the_feedback_flag_under_stable_keys(recorder, device_kind, monkeypatch, overlap):  # noqa: F811
    """step() and the overlap_backward hooks submit AVG | 0x1200, under the same keys every step."""
    from ddl.torch import Compression, cpp_backend as cb
    from ddl.torch import tensor_communicate as tc
    from ddl.torch.parallelism.data import data_parallelism_distributed_optimizer_wrapper
    monkeypatch.setattr(tc, 'memory_kind', lambda t, what='tensor': cb.MEMORY_DEVICE)
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Tanh(), torch.nn.Linear(5, 2))
    opt = data_parallelism_distributed_optimizer_wrapper(
        torch.optim.SGD(model.parameters(), lr=0.1), _Comm(), pin_host_gradients=False, fused_mean=True,
        compression=Compression.bf16_feedback, overlap_backward=overlap, bucket_bytes=None)
    keys = []
    for _ in range(2):
        del recorder.calls[:]
        opt.zero_grad()
        model(torch.randn(4, 6)).sum().backward()
        opt.step()
        assert sum(len(c['keys']) for c in recorder.calls) == 4
        assert all(c['op'] == cb.OP_AVG | 0x1200 for c in recorder.calls)
        keys.append(sorted(k for c in recorder.calls for k in c['keys']))
    assert keys[0] == keys[1] and len(set(keys[0])) == 4


def test_allreduce_gradient_refuses_feedback(recorder, monkeypatch):  # noqa: F811
    from ddl.torch import Compression, cpp_backend as cb
    from ddl.torch import tensor_communicate as tc
    monkeypatch.setattr(tc, 'memory_kind', lambda t, what='tensor': cb.MEMORY_DEVICE)
    monkeypatch.setattr(tc, 'stream_handle_for', lambda t: 0)
    g = torch.ones(2, 3)
    for comp in (Compression.fp16_feedback, Compression.bf16_feedback):
        with pytest.raises(ValueError, match='fresh'):
            tc.allreduce_gradient(g, _Comm(), compression=comp)
    assert recorder.calls == []  # nothing was submitted
    tc.allreduce_gradient(g, _Comm(), compression=Compression.bf16)  # the plain wire still works
    assert len(recorder.calls) == 1 and recorder.calls[0]['op'] == cb.OP_SUM | WIRE_BF16


def test_reset_error_feedback_raises_the_epoch(lib):
    from ddl.torch import config
    from ddl.torch.compression import reset_error_feedback
    assert 'wire_feedback_epoch' in config.KEYS and 'wire_feedback_epoch' not in config.SHARED
    old = config.get('wire_feedback_epoch')
    assert old >= 0
    try:
        reset_error_feedback()
        assert config.get('wire_feedback_epoch') == old + 1
        reset_error_feedback()
        assert lib.ddl_get_config(b'wire_feedback_epoch') == old + 2
        with config.override(wire_feedback_epoch=41):
            assert config.get('wire_feedback_epoch') == 41
        assert config.get('wire_feedback_epoch') == old + 2
    finally:
        config.set('wire_feedback_epoch', old)
