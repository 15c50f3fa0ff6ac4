"""The e4m3 wire over bfloat16 tensors through the engine on one GPU, bit for bit against _e4m3_bf16_helpers.py: thread
worlds whole and cut into sub-plans, the keyed handler at size 1, a round that mixes sources, the refusals."""
import ctypes

import numpy as np
import pytest
import torch

import _e4m3_bf16_helpers as h
import _e4m3_helpers as q8
from _bf16_native_helpers import assert_same, same_double
from _helpers import config
from test_e4m3_engine_gpu import DT_HALF, INVALID_ARGUMENT, OP_MIN, OP_SUM, THIRD, UNSUPPORTED_DTYPE, _floats, _stream, world  # noqa: F401

pytestmark = pytest.mark.gpu
LENS = q8.ENGINE_LENS


def _bf16(x):
    return torch.from_numpy(x.view(np.int16)).cuda().view(torch.bfloat16)


def _bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.mark.parametrize('P', [2, 3, 8])
def test_thread_world_is_the_model(lib, gpu, P):
    """SUM and AVG requests with and without factors, whole and cut by fusion_pipeline_bytes: the model's bits on every
    rank either way; the statistic is of the stored bf16 values, piece by piece."""
    k = len(LENS)
    ops, pre, post = [i % 2 for i in range(k)], [1.0, THIRD, 1.0, 0.5], [1.0, 1.0, THIRD, THIRD]
    xs = h.engine_inputs(P, LENS, q8.ENGINE_SEED)
    want = [h.allreduce([xs[r][i] for r in range(P)], ops[i], pre[i], post[i]) for i in range(k)]
    ins = [_bf16(x) for row in xs for x in row]
    for pipeline in (0, 4096):
        outs = [torch.full_like(t, 7.0) for t in ins]
        J, ncuts = ctypes.c_size_t(), ctypes.c_int()
        cs, ce, sq = (ctypes.c_size_t * 64)(), (ctypes.c_size_t * 64)(), (ctypes.c_double * (P * k))()
        with config(lib, tune=0, fusion_pipeline_bytes=pipeline):
            st = lib.ddl_testing_thread_fused_allreduce_e4m3_16(
                P, k, (ctypes.c_void_p * (P * k))(*[t.data_ptr() for t in ins]),
                (ctypes.c_void_p * (P * k))(*[t.data_ptr() for t in outs]), (ctypes.c_size_t * k)(*LENS), (ctypes.c_int * k)(*ops),
                h.DT_BFLOAT16, _floats(pre), _floats(post), _stream(), ctypes.byref(J), (ctypes.c_ubyte * k)(*([1] * k)), sq, cs,
                ce, 64, ctypes.byref(ncuts))
        assert st == 0, lib.ddl_last_error()
        torch.cuda.synchronize()
        assert (J.value > 1) == (pipeline > 0)
        cuts = [[ce[c] for c in range(ncuts.value) if cs[c] == i] for i in range(k)]
        assert all(c % q8.G == 0 for v in cuts for c in v)  # cuts fall between granules
        for j, out in enumerate(outs):
            assert_same(_bits(out), want[j % k], f'P={P} rank {j // k} request {j % k} ({J.value} sub-plans)')
            assert same_double(sq[j], h.sumsq(_bits(out), cuts[j % k])), j
    assert all(_bits(t).tobytes() == x.tobytes() for t, x in zip(ins, [x for row in xs for x in row])), 'an input was written'


def test_size_one_world(world, lib):
    """The keyed handler at P = 1. Off the shortcut: one quantization, a request cut by 64 KiB plans (256 granules:
    504-byte steps through the tensor), out != in; Compression.fp8 leaves a bf16 tensor as it is. On the shortcut the
    C-ABI's flagged bf16 request is its input, factors applied natively."""
    from ddl.torch import cpp_backend as cb
    from ddl.torch.compression import Compression
    from ddl.torch.tensor_communicate import allreduce_async
    x = h.rank_input(70_001, 21, specials=False)
    with config(lib, one_rank_shortcut=0, fusion_pipeline_bytes=0, fusion_threshold_bytes=64 << 10):
        src = _bf16(x)
        hd = allreduce_async(src, 'q16_cut', world, compression=Compression.fp8_all, op=cb.OP_AVG, prescale=THIRD,
                             postscale=3.0, sumsq=True)
        out = hd.wait(60)
        assert out.data_ptr() != src.data_ptr() and _bits(src).tobytes() == x.tobytes()
        want = h.allreduce([x], q8.OP_AVG, THIRD, 3.0)
        assert_same(_bits(out), want, 'request cut by 64 KiB plans')
        assert same_double(hd.sumsq, h.sumsq(want, range(256 * q8.G, x.size, 256 * q8.G)))  # a plan's unpack is a piece
        out = allreduce_async(_bf16(x), 'q16_plain_kind', world, compression=Compression.fp8).wait(60)
        assert _bits(out).tobytes() == x.tobytes()
    with config(lib, one_rank_shortcut=1):
        src, out = _bf16(x), torch.empty(x.size, dtype=torch.bfloat16, device='cuda')
        done = cb.DONE_FN(lambda status, user: None)
        assert lib.ddl_allreduce_submit_mem(world.id, b'q16_short', src.data_ptr(), out.data_ptr(), x.size, h.DT_BFLOAT16,
                                            OP_SUM | q8.WIRE_E4M3, cb.MEMORY_DEVICE, _stream(), done, None) == 0
        assert lib.ddl_wait_all(world.id) == 0
        torch.cuda.synchronize()
        assert _bits(out).tobytes() == x.tobytes()


def test_mixed_round(world, lib):
    """One batch under Compression.fp8_all holding an fp32 and a bf16 tensor — one submission, so one round, whose two
    e4m3 groups differ only in the key's source dtype — with a plain bf16 request right behind it. All three are the
    model's, and the first and the third are what they are without the second."""
    from ddl.torch.compression import Compression
    from ddl.torch.tensor_communicate import allreduce_async, allreduce_async_batch
    f, b, p = q8.rank_input(4099, 31, specials=False), h.rank_input(4099, 32), h.rank_input(777, 33)

    def round_(tag, with_bf16):
        ts = [torch.from_numpy(f).cuda()] + ([_bf16(b)] if with_bf16 else [])
        with config(lib, one_rank_shortcut=0):
            hs = allreduce_async_batch(ts, [f'q16_mix_{tag}_{i}' for i in range(len(ts))], world, compression=Compression.fp8_all)
            hs.append(allreduce_async(_bf16(p), f'q16_mix_{tag}_p', world))
            return [x.wait(60) for x in hs]
    a0, c0 = round_('without', False)
    a1, b1, c1 = round_('with', True)
    assert a1.cpu().numpy().tobytes() == q8.allreduce([f]).tobytes() == a0.cpu().numpy().tobytes()
    assert_same(_bits(b1), h.allreduce([b]), 'the bf16-source request')
    assert _bits(c1).tobytes() == p.tobytes() == _bits(c0).tobytes()


def test_refusals(world, lib):
    """What stays refused, before anything is registered; a plain request works afterwards."""
    from ddl.torch import cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async
    done = cb.DONE_FN(lambda status, user: None)
    b16 = torch.ones(16, dtype=torch.bfloat16, device='cuda')
    f16 = torch.ones(16, dtype=torch.float16, device='cuda')
    hb16 = torch.ones(16, dtype=torch.bfloat16)
    Q, BF = q8.WIRE_E4M3, h.DT_BFLOAT16

    def submit(t, dt, op, mem=cb.MEMORY_DEVICE):
        return lib.ddl_allreduce_submit_mem(world.id, b'q16_refused', t.data_ptr(), t.data_ptr(), 16, dt, op, mem, _stream(),
                                            done, None)
    assert submit(f16, DT_HALF, OP_SUM | Q) == UNSUPPORTED_DTYPE
    assert submit(b16, BF, OP_SUM | Q | cb.WIRE_E4M3_FEEDBACK) == UNSUPPORTED_DTYPE
    assert submit(b16, BF, OP_SUM | cb.WIRE_BF16) == UNSUPPORTED_DTYPE  # the 16-bit wires stay fp32-only
    assert submit(hb16, BF, OP_SUM | Q, cb.MEMORY_HOST) == INVALID_ARGUMENT
    assert submit(b16, BF, OP_MIN | Q) == INVALID_ARGUMENT
    assert lib.ddl_allreduce(world.id, b16.data_ptr(), b16.data_ptr(), 16, BF, OP_SUM | Q, _stream()) == INVALID_ARGUMENT
    assert lib.ddl_wait_all(world.id) == 0
    assert (b16 == 1).all() and (hb16 == 1).all()  # nothing ran
    x = torch.randn(1000, device='cuda')
    assert torch.equal(allreduce_async(x, 'q16_after_refusals', world).wait(60), x)
