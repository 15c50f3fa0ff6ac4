"""The sum of squares through the engine on one GPU: the keyed path's FusionPipe on every virtual rank
(thread world) with per-segment wishes, unpipelined and cut into sub-plans, uncompressed and over the
bf16 wire; the size-1 world's keyed requests (direct plans, fused plans, requests spanning plans, the
one-rank shortcut); the refusals.

Expected: the outputs are, byte for byte, what the entries without the statistic give; every sum of
squares is, bit for bit, _sumsq_helpers.mirror of that output with the cuts the run reports, and the
same on every virtual rank."""
import ctypes
import math
import struct

import numpy as np
import pytest
import torch

from _helpers import config
from _sumsq_helpers import mirror

pytestmark = pytest.mark.gpu
DT_FLOAT, DT_INT32, DT_BFLOAT16, DT_HALF = 1, 3, 14, 19
OP_SUM, OP_AVG, OP_MIN, OP_MAX = 0, 1, 3, 4
INVALID_ARGUMENT, UNSUPPORTED_DTYPE = 3, 4
ELEMS = [5, 300, 70_001, 4099, 1, 200_000, 513]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(v):
    return struct.pack('<d', v)


@pytest.mark.parametrize('pipeline', [0, 256 << 10], ids=['unpipelined', 'subplans'])
@pytest.mark.parametrize('wire', [0, DT_BFLOAT16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('P', [2, 3])
def test_thread_world_fused(lib, gpu, P, wire, pipeline):
    k = len(ELEMS)
    ops = [i % 2 for i in range(k)]            # SUM, AVG, SUM, ...
    want = [1 if i % 4 < 2 else 0 for i in range(k)]  # wanted, wanted, not, not, ...: every (op, wish) pair
    assert {(o, w) for o, w in zip(ops, want)} == {(0, 0), (0, 1), (1, 0), (1, 1)} and want[2] + want[5] == 1
    rng = np.random.default_rng(100 * P + wire)
    xs = [[rng.standard_normal(n).astype(np.float32) for n in ELEMS] for _ in range(P)]
    ins = [[torch.from_numpy(x).to(gpu) for x in row] for row in xs]
    S = (ctypes.c_void_p * (P * k))(*[t.data_ptr() for row in ins for t in row])
    n_arr = (ctypes.c_size_t * k)(*ELEMS)
    c_ops = (ctypes.c_int * k)(*ops)

    def outputs():
        outs = [[torch.zeros_like(t) for t in row] for row in ins]
        return outs, (ctypes.c_void_p * (P * k))(*[t.data_ptr() for row in outs for t in row])
    with config(lib, reference_order=1, tune=0, fusion_pipeline_bytes=pipeline):
        ref, D = outputs()
        J0 = ctypes.c_size_t()
        if wire:
            st = lib.ddl_testing_thread_fused_allreduce_wire(P, k, S, D, n_arr, c_ops, wire, _stream(), ctypes.byref(J0))
        else:
            st = lib.ddl_testing_thread_fused_allreduce_ops(P, k, S, D, (ctypes.c_size_t * k)(*[4 * n for n in ELEMS]),
                                                            c_ops, DT_FLOAT, _stream(), ctypes.byref(J0))
        assert st == 0, lib.ddl_last_error()
        torch.cuda.synchronize()
        got, D = outputs()
        J, ncuts = ctypes.c_size_t(), ctypes.c_int()
        sq = (ctypes.c_double * (P * k))(*([-1.0] * (P * k)))
        cs, ce = (ctypes.c_size_t * 64)(), (ctypes.c_size_t * 64)()
        st = lib.ddl_testing_thread_fused_allreduce_sumsq(P, k, S, D, n_arr, c_ops, wire, _stream(), ctypes.byref(J),
                                                          (ctypes.c_ubyte * k)(*want), sq, cs, ce, 64, ctypes.byref(ncuts))
        assert st == 0, lib.ddl_last_error()
        torch.cuda.synchronize()
    assert J.value == J0.value and (J.value > 1) == bool(pipeline)
    assert 0 <= ncuts.value <= 64
    cuts = {}
    for c in range(ncuts.value):
        cuts.setdefault(cs[c], []).append(ce[c])
    if pipeline:  # a segment above the sub-plan size is certainly cut
        big = 2 if want[2] else 5
        assert cuts.get(big), cuts
    else:
        assert not cuts
    for r in range(P):
        for i in range(k):
            out = got[r][i].cpu().numpy()
            assert out.tobytes() == ref[r][i].cpu().numpy().tobytes(), f'rank {r} segment {i}: the output changed'
            v = sq[r * k + i]
            if want[i]:
                m = mirror(out, bool(wire), cuts.get(i, ()))
                assert math.isfinite(m) and _bits(v) == _bits(m), (r, i, v, m, cuts.get(i))
                assert _bits(v) == _bits(sq[i]), f'segment {i}: rank {r} differs from rank 0'
            else:
                assert _bits(v) == _bits(0.0)


@pytest.fixture(scope='module')
def world(gpu):
    from ddl.torch.communicator import Communicator
    return Communicator.world()


@pytest.mark.parametrize('shortcut', [1, 0])
def test_size_one_world(world, lib, shortcut):
    """Keyed requests at P = 1 with and without the one-rank shortcut: a single request (the direct
    plan), a batch (one fused plan, mixed wishes, SUM and AVG), a request spanning plans, an empty one."""
    from ddl.torch import cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async, allreduce_async_batch
    torch.manual_seed(11)
    tag = f'sq1_{shortcut}'
    with config(lib, one_rank_shortcut=shortcut, fusion_pipeline_bytes=0):
        x = torch.randn(70_001, device='cuda')
        h = allreduce_async(x, f'{tag}_single', world, sumsq=True)
        out = h.wait(60)
        assert torch.equal(out, x) and _bits(h.sumsq) == _bits(mirror(x.cpu().numpy(), False))
        h = allreduce_async(x[1:], f'{tag}_misaligned', world, op=cb.OP_AVG, sumsq=True)  # 4-byte aligned only
        assert torch.equal(h.wait(60), x[1:]) and _bits(h.sumsq) == _bits(mirror(x[1:].cpu().numpy(), False))
        e = torch.empty(0, device='cuda')
        h = allreduce_async(e, f'{tag}_empty', world, sumsq=True)
        h.wait(60)
        assert _bits(h.sumsq) == _bits(0.0)
        ts = [torch.randn(n, device='cuda') for n in (5, 300, 4099, 70_001, 1)]
        ts[2][7] = math.inf
        wishes = [True, False, True, True, False]
        hs = allreduce_async_batch(ts, [f'{tag}_b{i}' for i in range(len(ts))], world, outputs=ts, op=cb.OP_AVG,
                                   sumsq=wishes)
        for t, hh, w in zip(ts, hs, wishes):
            hh.wait(60)
            assert (hh.sumsq is not None) == w
            if w:
                assert _bits(hh.sumsq) == _bits(mirror(t.cpu().numpy(), False)), (t.numel(), hh.sumsq)
        assert hs[2].sumsq == math.inf and math.isfinite(hs[3].sumsq)
        # 64 KiB plans: the last request spans plans, cut where the plans end in the round's byte stream
        with config(lib, fusion_threshold_bytes=64 << 10):
            ys = [torch.randn(n, device='cuda') for n in (5, 300, 70_001)]
            hs = allreduce_async_batch(ys, [f'{tag}_p{i}' for i in range(3)], world, sumsq=True)
            outs = [hh.wait(60) for hh in hs]
        before = 4 * (5 + 300)
        cuts = [(j * (64 << 10) - before) // 4 for j in range(1, 6) if (j * (64 << 10) - before) // 4 < 70_001]
        assert len(cuts) == 4
        for y, o, hh, c in zip(ys, outs, hs, ((), (), cuts)):
            assert torch.equal(o, y) and _bits(hh.sumsq) == _bits(mirror(y.cpu().numpy(), False, c)), (y.numel(), hh.sumsq)


def test_refusals(world, lib):
    """A non-NULL sumsq with another dtype: UNSUPPORTED_DTYPE; with MIN / MAX: INVALID_ARGUMENT; nothing
    is registered and the communicator works afterwards. A NULL sumsq is the plain submission."""
    from ddl.torch import cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async
    done = cb.DONE_FN(lambda status, user: None)
    v = (ctypes.c_double * 1)(-1.0)
    ptrs = (ctypes.c_void_p * 1)(ctypes.addressof(v))
    keys, users, n1 = (ctypes.c_char_p * 1)(b'sq_refused'), (ctypes.c_void_p * 1)(None), (ctypes.c_size_t * 1)(16)
    for dt, tdt, op, want in ((DT_INT32, torch.int32, OP_SUM, UNSUPPORTED_DTYPE),
                              (DT_HALF, torch.float16, OP_AVG, UNSUPPORTED_DTYPE),
                              (DT_FLOAT, torch.float32, OP_MIN, INVALID_ARGUMENT),
                              (DT_FLOAT, torch.float32, OP_MAX, INVALID_ARGUMENT),
                              (DT_INT32, torch.int32, OP_MAX, UNSUPPORTED_DTYPE)):
        d = torch.ones(16, dtype=tdt, device='cuda')
        one = (ctypes.c_void_p * 1)(d.data_ptr())
        assert lib.ddl_allreduce_submit_sumsq(world.id, b'sq_refused', d.data_ptr(), d.data_ptr(), 16, dt, op, _stream(),
                                              done, None, v) == want
        assert lib.ddl_last_error()
        assert lib.ddl_allreduce_submit_batch_sumsq(world.id, 1, keys, one, one, n1, (ctypes.c_int * 1)(dt), op,
                                                    _stream(), done, users, ptrs) == want
    # the deployment form: the bit in `op` and a ddl_sumsq_arg as the user pointer
    arg = cb.SumsqArg(None, ctypes.addressof(v))
    d = torch.ones(16, dtype=torch.int32, device='cuda')
    one, h32 = (ctypes.c_void_p * 1)(d.data_ptr()), torch.ones(16)
    for fn_args, want in (
            ((d.data_ptr(), d.data_ptr(), 16, DT_INT32, OP_SUM | cb.SUMSQ, cb.MEMORY_DEVICE), UNSUPPORTED_DTYPE),
            ((h32.data_ptr(), h32.data_ptr(), 16, DT_FLOAT, OP_SUM | cb.SUMSQ, cb.MEMORY_HOST), INVALID_ARGUMENT)):
        assert lib.ddl_allreduce_submit_mem(world.id, b'sq_refused', *fn_args, _stream(), done, ctypes.addressof(arg)) == want
    f32 = torch.ones(16, device='cuda')
    assert lib.ddl_allreduce_submit_mem(world.id, b'sq_refused', f32.data_ptr(), f32.data_ptr(), 16, DT_FLOAT,
                                        OP_SUM | cb.SUMSQ, cb.MEMORY_DEVICE, _stream(), done, None) == INVALID_ARGUMENT
    assert lib.ddl_allreduce_submit_batch_mem(world.id, 1, keys, one, one, n1, (ctypes.c_int * 1)(DT_FLOAT),
                                              OP_SUM | cb.SUMSQ, cb.MEMORY_DEVICE, _stream(), done, None) == INVALID_ARGUMENT
    assert lib.ddl_allreduce(world.id, f32.data_ptr(), f32.data_ptr(), 16, DT_FLOAT, OP_SUM | cb.SUMSQ,
                             _stream()) == INVALID_ARGUMENT
    assert lib.ddl_wait_all(world.id) == 0 and v[0] == -1.0  # nothing was registered, nothing written
    # every sumsq NULL: ddl_allreduce_submit / _submit_batch, also for what the statistic refuses
    d = torch.arange(16, dtype=torch.int32, device='cuda')
    one = (ctypes.c_void_p * 1)(d.data_ptr())
    assert lib.ddl_allreduce_submit_sumsq(world.id, b'sq_null', d.data_ptr(), d.data_ptr(), 16, DT_INT32, OP_MAX,
                                          _stream(), done, None, None) == 0
    assert lib.ddl_allreduce_submit_batch_sumsq(world.id, 1, keys, one, one, n1, (ctypes.c_int * 1)(DT_INT32), OP_SUM,
                                                _stream(), done, users, None) == 0
    assert lib.ddl_wait_all(world.id) == 0
    x = torch.randn(1000, device='cuda')
    h = allreduce_async(x, 'sq_after_refusal', world, sumsq=True)
    assert torch.equal(h.wait(60), x) and _bits(h.sumsq) == _bits(mirror(x.cpu().numpy(), False))
