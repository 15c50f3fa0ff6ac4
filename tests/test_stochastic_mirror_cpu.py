"""Stochastic rounding of the bf16 wire (DDL_ALLREDUCE_WIRE_STOCHASTIC) without a GPU: the constants and the
Python surface, the rule of include/ddl_amd.h as tests/_stochastic_helpers.py restates it, the generator's
statistics at fixed stream keys (fixed computations, nothing random at test time) and the host mix."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _stochastic_helpers as sh
from _helpers import DT_BFLOAT16
from _wire_helpers import narrow, widen
from test_wire_mirror_cpu import _Comm, _Solo, device_kind, recorder  # noqa: F401 (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_and_python_surface():
    from ddl.torch import Compression, config, cpp_backend as cb
    from ddl.torch.compression import set_stochastic_seed, wire_flag  # noqa: F401  (the name exists)
    assert cb.WIRE_STOCHASTIC == sh.WIRE_STOCHASTIC == 0x8000
    with open(os.path.join(ROOT, 'include', 'ddl_amd.h')) as fh:
        header = fh.read()
    assert re.search(r'DDL_ALLREDUCE_WIRE_STOCHASTIC\s*=\s*0x8000\b', header)
    for other in (cb.WIRE_FP16, cb.WIRE_BF16, cb.WIRE_FEEDBACK, cb.SUMSQ, cb.SCALE, 0x80, 0x400, 0x800, 0xff):
        assert not cb.WIRE_STOCHASTIC & other  # a free bit, outside the op's low bits
    k = Compression.bf16_stochastic
    assert wire_flag(k) == cb.WIRE_BF16 | cb.WIRE_STOCHASTIC
    assert repr(k) == 'Compression.bf16_stochastic'
    assert k.stochastic and not k.feedback
    for other in (Compression.none, Compression.fp16, Compression.bf16, Compression.fp16_feedback,
                  Compression.bf16_feedback):
        assert not other.stochastic
    with pytest.raises(TypeError, match='bf16_stochastic'):
        wire_flag('bf16_stochastic')
    assert 'wire_stochastic_seed' in config.KEYS and 'wire_stochastic_seed' not in config.SHARED


def test_allreduce_gradient_refuses_it(recorder, monkeypatch):  # noqa: F811
    """Its compressed requests get a fresh name per call: one entry of the engine's per-key map per call."""
    from ddl.torch import Compression, cpp_backend as cb
    from ddl.torch import tensor_communicate as tc
    monkeypatch.setattr(tc, 'memory_kind', lambda t, what='tensor': cb.MEMORY_DEVICE)
    monkeypatch.setattr(tc, 'stream_handle_for', lambda t: 0)
    with pytest.raises(ValueError, match='bf16_stochastic'):
        tc.allreduce_gradient(torch.ones(2, 3), _Comm(), compression=Compression.bf16_stochastic)
    assert recorder.calls == []  # nothing was submitted
    assert 'bf16_stochastic' in tc.allreduce_gradient.__doc__


def test_flag_reaches_the_engine_for_fp32_device_requests_only(recorder, device_kind):  # noqa: F811
    from ddl.torch import Compression, cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async, allreduce_async_batch
    dev32, dev16, host32 = torch.ones(5), torch.ones(5, dtype=torch.float16), torch.ones(5)
    device_kind += [dev32, dev16]
    k = Compression.bf16_stochastic
    for op in (cb.OP_SUM, cb.OP_AVG):
        allreduce_async(dev32, 'a', _Comm(), output=dev32, op=op, compression=k).wait(5)
        assert recorder.calls[-1] == {'keys': ['a'], 'dts': [cb.DT_FLOAT], 'op': op | 0x8200, 'mem': cb.MEMORY_DEVICE}
        allreduce_async(dev16, 'b', _Comm(), output=dev16, op=op, compression=k).wait(5)
        assert recorder.calls[-1]['op'] == op  # not fp32: no wire bits at all
        allreduce_async(host32, 'c', _Comm(), output=host32, op=op, compression=k).wait(5)
        assert recorder.calls[-1] == {'keys': ['c'], 'dts': [cb.DT_FLOAT], 'op': op, 'mem': cb.MEMORY_HOST}
    allreduce_async(dev32, 'a', _Solo(), output=dev32, compression=k).wait(5)
    assert recorder.calls[-1]['op'] == cb.OP_SUM  # size 1 with the shortcut: nothing is communicated
    del recorder.calls[:]
    ts = [dev32, dev16, host32]
    for h in allreduce_async_batch(ts, ['k0', 'k1', 'k2'], _Comm(), outputs=ts, op=cb.OP_AVG, compression=k):
        h.wait(5)
    assert {'keys': ['k0'], 'dts': [cb.DT_FLOAT], 'op': cb.OP_AVG | 0x8200, 'mem': cb.MEMORY_DEVICE} in recorder.calls
    assert sorted(c['op'] for c in recorder.calls) == [cb.OP_AVG, cb.OP_AVG, cb.OP_AVG | 0x8200]
    with pytest.raises(ValueError):  # MIN / MAX take no compression
        allreduce_async(dev32, 'a', _Comm(), output=dev32, op=cb.OP_MAX, compression=k)


@pytest.mark.parametrize('overlap', [False, True])
def test_wrapper_carries_the_flag_under_stable_keys(recorder, device_kind, monkeypatch, overlap):  # noqa: F811
    """step() and the overlap_backward hooks submit AVG | 0x8200, under the same keys every step."""
    from ddl.torch import Compression, cpp_backend as cb
    from ddl.torch import tensor_communicate as tc
    from ddl.torch.parallelism.data import data_parallelism_distributed_optimizer_wrapper
    monkeypatch.setattr(tc, 'memory_kind', lambda t, what='tensor': cb.MEMORY_DEVICE)
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Tanh(), torch.nn.Linear(5, 2))
    opt = data_parallelism_distributed_optimizer_wrapper(
        torch.optim.SGD(model.parameters(), lr=0.1), _Comm(), pin_host_gradients=False, fused_mean=True,
        compression=Compression.bf16_stochastic, overlap_backward=overlap, bucket_bytes=None)
    keys = []
    for _ in range(2):
        del recorder.calls[:]
        opt.zero_grad()
        model(torch.randn(4, 6)).sum().backward()
        opt.step()
        assert sum(len(c['keys']) for c in recorder.calls) == 4
        assert all(c['op'] == cb.OP_AVG | 0x8200 for c in recorder.calls)
        keys.append(sorted(k for c in recorder.calls for k in c['keys']))
    assert keys[0] == keys[1] and len(set(keys[0])) == 4


def test_round_up_count_is_the_low_half():
    """For u = 0x3f800000 | k exactly k of the 65536 values of r round up: probability k / 65536."""
    r = np.arange(65536, dtype=np.uint32)
    up = np.empty(65536, np.int64)
    for k0 in range(0, 65536, 256):  # 256 values of k at a time
        u = (np.uint32(0x3f800000) | np.arange(k0, k0 + 256, dtype=np.uint32))[:, None]
        w = sh.round_bits(np.broadcast_to(u, (256, 65536)), np.broadcast_to(r, (256, 65536)))
        assert ((w == 0x3f80) | (w == 0x3f81)).all()
        up[k0:k0 + 256] = (w == 0x3f81).sum(axis=1)
    assert np.array_equal(up, np.arange(65536))


def test_edge_patterns():
    u = sh.EDGE_BITS
    lo, hi = sh.round_bits(u, np.zeros(u.size, np.uint32)), sh.round_bits(u, np.full(u.size, 0xffff, np.uint32))
    # +-0 stay +-0 and the sign never changes, whatever r
    assert lo[0] == hi[0] == 0x0000 and lo[1] == hi[1] == 0x8000
    num = (u & 0x7fffffff) <= 0x7f800000  # (a NaN's sign is the cast's, not pinned)
    assert ((lo >> 15) == (u >> 31))[num].all() and ((hi >> 15) == (u >> 31))[num].all()
    # the smallest fp32 subnormal: to zero, or to the smallest bf16 subnormal with probability 2^-16
    assert (lo[2], hi[2], lo[3], hi[3]) == (0x0000, 0x0001, 0x8000, 0x8001)
    # the largest finite value becomes inf for every r > 0
    every = sh.round_bits(np.full(65536, 0x7f7fffff, np.uint32), np.arange(65536, dtype=np.uint32))
    assert every[0] == 0x7f7f and (every[1:] == 0x7f80).all()
    assert hi[5] == 0xff80
    # inf and NaN: the round-to-nearest result, independent of r
    special = np.flatnonzero((u & 0x7f800000) == 0x7f800000)
    assert special.size == 6
    rne = narrow(DT_BFLOAT16, u.view(np.float32))
    for r in (0, 1, 0x7fff, 0x8000, 0xffff):
        w = sh.round_bits(u, np.full(u.size, r, np.uint32))
        assert np.array_equal(w[special], rne[special])
    assert lo[6] == 0x7f80 and lo[7] == 0xff80 and (((lo[8:12] & 0x7fff) > 0x7f80).all())
    # subnormal to normal and a carry into the next binade are the same formula
    assert (lo[14], hi[14]) == (0x007f, 0x0080) and (lo[15], hi[15]) == (0x3f80, 0x3f81)
    # a value already on the bf16 grid never moves
    grid = np.array([0x3f800000, 0xc0490000, 0x00010000, 0x7f7f0000], np.uint32)
    for r in (0, 0xffff):
        assert np.array_equal(sh.round_bits(grid, np.full(4, r, np.uint32)), (grid >> 16).astype(np.uint16))


def test_random_bits_are_a_function_of_the_index():
    """R(S, i) of a piece that starts anywhere equals the whole tensor's bits at those indices, also
    across 2^32 and 2^33 (hi32 of the pair index changes), and both halves of a word are used."""
    S = sh.STREAMS[2]
    whole = sh.random_bits(S, np.arange(4096, dtype=np.uint64))
    assert whole.max() < 65536 and len(set(whole.tolist())) > 3800
    for first in (1, 7, 8, 128, 513):
        assert np.array_equal(sh.random_bits(S, np.uint64(first) + np.arange(100, dtype=np.uint64)), whole[first:first + 100])
    x = np.linspace(-3, 3, 300, dtype=np.float32)
    assert np.array_equal(sh.sr(x[37:], S, first=37), sh.sr(x, S)[37:])
    big = np.uint64(2 ** 33 - 6) + np.arange(12, dtype=np.uint64)
    one_by_one = np.array([int(sh.random_bits(S, np.array([i], np.uint64))[0]) for i in big])
    assert np.array_equal(sh.random_bits(S, big), one_by_one)
    assert not np.array_equal(sh.random_bits(S, big), sh.random_bits(S, big - np.uint64(2 ** 33)))


@pytest.mark.parametrize('S', sh.STREAMS, ids=hex)
def test_mean_error_is_unbiased(S):
    """65536 elements of 1 + 2**-10: the mean error within 5 standard errors of 0 (measured with these keys:
    within 2), where the plain cast is off by 2**-10 = 18 sigma of ONE element at every element."""
    n = 65536
    err = sh.mean_error(S, n)
    print(f'S={S:#x}: mean error {err:.3e} = {err / (sh.SIGMA / np.sqrt(n)):+.2f} standard errors')
    assert abs(err) <= 5 * sh.SIGMA / np.sqrt(n)
    w = widen(DT_BFLOAT16, sh.sr(np.full(n, sh.VALUE, np.float32), S))
    assert set(w.tolist()) == {1.0, 1.0078125}


def test_sequence_numbers_of_one_key_are_unbiased():
    """64 consecutive sequence numbers of one key on 4096 elements: every step within 5 standard errors, and
    so is the mean over all of them; no two steps share their bits."""
    n, steps = 4096, 64
    streams = [sh.stream(0, 0, 'stochastic/seq', t) for t in range(steps)]
    assert len(set(streams)) == steps
    errs = np.array([sh.mean_error(S, n) for S in streams])
    print('worst step', np.abs(errs).max() / (sh.SIGMA / np.sqrt(n)), 'overall', errs.mean() / (sh.SIGMA / np.sqrt(n * steps)))
    assert (np.abs(errs) <= 5 * sh.SIGMA / np.sqrt(n)).all()
    assert abs(errs.mean()) <= 5 * sh.SIGMA / np.sqrt(n * steps)
    ws = {sh.sr(np.full(n, sh.VALUE, np.float32), S).tobytes() for S in streams}
    assert len(ws) == steps


def test_host_mix():
    """Pinned values of the mix (computed from the header's formulas by hand-written Python integers), its
    sensitivity to every input, and the engine's own mix where the testing library is built."""
    assert sh.fnv1a64(b'') == 0xcbf29ce484222325 and sh.fnv1a64(b'a') == 0xaf63dc4c8601ec8c
    assert sh.mix64(0) == 0xe220a8397b1dcdaf  # splitmix64's first output from state 0
    base = sh.stream(0, 0, 'w', 0)
    others = [sh.stream(1, 0, 'w', 0), sh.stream(0, 1, 'w', 0), sh.stream(0, 0, 'x', 0), sh.stream(0, 0, 'w', 1),
              sh.stream(2 ** 64 - 1, 0, 'w', 0)]
    assert len({base, *others}) == 6
    for o in others:  # a one-bit change of an input moves about half of S's bits
        assert 16 <= bin(base ^ o).count('1') <= 48
    from conftest import TESTING_LIB
    if not os.path.exists(TESTING_LIB):
        return
    from ddl.torch.cpp_backend import CPPBackend
    lib = CPPBackend.c_api()
    for seed, rank, key, n in [(0, 0, b'w', 0), (2 ** 64 - 1, 7, b'layer.3/weight', 12345), (12345, 2, b'', 2 ** 40)]:
        S = ctypes.c_ulonglong()
        assert lib.ddl_testing_stochastic_stream(seed, rank, key, n, ctypes.byref(S)) == 0
        assert S.value == sh.stream(seed, rank, key, n)
