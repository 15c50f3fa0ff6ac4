"""The e4m3 wire through the engine on one GPU: the keyed path's FusionPipe and the production executor on every
virtual rank (thread world) at P = 2, 3, 8 and 16 on the default schedule, unpipelined and cut into sub-plans; every
configured schedule and order mode at P = 2, 3 and 8; the happens-before check; the keyed handler at size 1 with the
data plane on; the refusals. Everything is compared bit for bit with the CPU model of _e4m3_helpers.py (a NaN must
be a NaN)."""
import ctypes
import math
import struct

import numpy as np
import pytest
import torch

import _e4m3_helpers as q8
from _avg_helpers import assert_same
from _helpers import config
from _sumsq_helpers import mirror

pytestmark = pytest.mark.gpu
DT_FLOAT, DT_INT32, DT_HALF = 1, 3, 19
OP_SUM, OP_AVG, OP_MIN, OP_MAX = 0, 1, 3, 4
INVALID_ARGUMENT, UNSUPPORTED_DTYPE = 3, 4
THIRD = float(np.float32(1) / np.float32(3))
LENS = q8.ENGINE_LENS


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(v):
    return struct.pack('<d', v)


def _floats(values):
    return (ctypes.c_float * len(values))(*[float(v) for v in values])


def _thread_run(lib, gpu, P, xs, ops, pre=None, post=None, want=None, status=0):
    """One fused e4m3 allreduce of the thread world over xs[r][i]. Returns (outputs [r][i], sub-plans, sums of
    squares or None, cuts by segment)."""
    k = len(xs[0])
    ins = [[torch.from_numpy(x).to(gpu) for x in row] for row in xs]
    outs = [[torch.full_like(t, 7.0) for t in row] for row in ins]
    S = (ctypes.c_void_p * (P * k))(*[t.data_ptr() for row in ins for t in row])
    D = (ctypes.c_void_p * (P * k))(*[t.data_ptr() for row in outs for t in row])
    n_arr = (ctypes.c_size_t * k)(*[len(x) for x in xs[0]])
    J, ncuts = ctypes.c_size_t(), ctypes.c_int()
    cs, ce = (ctypes.c_size_t * 64)(), (ctypes.c_size_t * 64)()
    sq = (ctypes.c_double * (P * k))(*([-1.0] * (P * k))) if want is not None else None
    st = lib.ddl_testing_thread_fused_allreduce_e4m3(
        P, k, S, D, n_arr, (ctypes.c_int * k)(*ops), _floats(pre) if pre is not None else None,
        _floats(post) if post is not None else None, _stream(), ctypes.byref(J),
        (ctypes.c_ubyte * k)(*want) if want is not None else None, sq, cs, ce, 64, ctypes.byref(ncuts))
    assert st == status, lib.ddl_last_error()
    torch.cuda.synchronize()
    cuts = {}
    for c in range(ncuts.value):
        cuts.setdefault(cs[c], []).append(ce[c])
    for row_in, row in zip(ins, xs):
        for t, x in zip(row_in, row):
            assert t.cpu().numpy().tobytes() == x.tobytes(), 'an input was written'
    return [[t.cpu().numpy() for t in row] for row in outs], J.value, (list(sq) if sq is not None else None), cuts


@pytest.fixture(scope='module')
def models():
    """The model's results of the shared inputs, computed once per (P, variant)."""
    cache = {}

    def get(P, ops, pre, post):
        key = (P, tuple(ops), tuple(pre), tuple(post))
        if key not in cache:
            xs = q8.engine_inputs(P, LENS, q8.ENGINE_SEED)
            cache[key] = (xs, [q8.allreduce([xs[r][i] for r in range(P)], ops[i], pre[i], post[i])
                               for i in range(len(LENS))])
        return cache[key]
    return get


@pytest.mark.parametrize('P', q8.ENGINE_RANKS)
def test_thread_world_is_the_model(lib, gpu, models, P):
    """SUM and AVG requests with and without factors, unpipelined and cut by fusion_pipeline_bytes: the model's
    bits on every rank, and the same bits either way; the statistic is the canonical uncompressed sum of `out`."""
    k = len(LENS)
    ops = [i % 2 for i in range(k)]
    pre = [1.0, THIRD, 1.0, 0.5]
    post = [1.0, 1.0, THIRD, THIRD]
    xs, want = models(P, ops, pre, post)
    runs = []
    for pipeline in (0, 4096):
        with config(lib, tune=0, fusion_pipeline_bytes=pipeline):
            runs.append(_thread_run(lib, gpu, P, xs, ops, pre, post, [1] * k))
    assert runs[0][1] == 1 and runs[1][1] > 1
    for got, J, sq, cuts in runs:
        for r in range(P):
            for i in range(k):
                assert_same(DT_FLOAT, got[r][i], want[i], f'P={P} rank {r} request {i} ({J} sub-plans)')
                assert got[r][i].tobytes() == got[0][i].tobytes(), f'rank {r} differs from rank 0'
                m = mirror(got[r][i], False, cuts.get(i, ()))
                v = sq[r * k + i]
                assert (math.isnan(v) and math.isnan(m)) or _bits(v) == _bits(m), (r, i, v, m)
    for a, b in zip(runs[0][0], runs[1][0]):
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes(), 'the pipeline cuts changed bits'
    assert all(c % q8.G == 0 for v in runs[1][3].values() for c in v)  # cuts fall between granules


@pytest.mark.parametrize('ref_order', [0, 1])
@pytest.mark.parametrize('algo', [0, 1, 2, 3, 4], ids=['ring', 'direct', 'oneshot', 'gatherfold', 'directgather'])
def test_bits_do_not_depend_on_the_schedule(lib, gpu, models, algo, ref_order):
    """Every configured schedule, sliced finely, in either order mode, at P = 2 (the ring's single step), P = 3 and
    P = 8 (a ring becomes the direct schedule): the model's bits. (The thread world runs the configured schedule; the
    tuner is a communicator's: tests/_mp_e4m3_worker.py check_e4m3_tuned.)"""
    k = len(LENS)
    ones = [1.0] * k
    for P in (2, 3, 8):
        xs, want = models(P, [OP_SUM] * k, ones, ones)
        with config(lib, tune=0, fusion_pipeline_bytes=0, algo=algo, reference_order=ref_order, slice_bytes=2048,
                    max_slices=8):
            got, _, _, _ = _thread_run(lib, gpu, P, xs, [OP_SUM] * k)
        for r in range(P):
            for i in range(k):
                assert_same(DT_FLOAT, got[r][i], want[i], f'algo {algo} P={P} rank {r} request {i}')
                assert got[r][i].tobytes() == got[0][i].tobytes()


def test_thread_world_is_race_free(lib, gpu):
    """The happens-before check over a pipelined plan with factors and the statistic, in every rank's own buffers."""
    P, k = 3, len(LENS)
    xs = [[np.full(n, 1.0 + r, np.float32) for n in LENS] for r in range(P)]
    counts, report = (ctypes.c_longlong * 5)(), ctypes.create_string_buffer(1 << 14)
    with config(lib, tune=0, fusion_pipeline_bytes=4096):
        assert lib.ddl_testing_dep_trace(1) == 0
        try:
            got, J, _, _ = _thread_run(lib, gpu, P, xs, [OP_AVG] * k, [0.5] * k, [2.0] * k, [1] * k)
            assert J > 1
        finally:
            torch.cuda.synchronize()
            assert lib.ddl_testing_dep_trace(0) == 0
    assert lib.ddl_testing_dep_check(counts, report, len(report)) == 0, lib.ddl_last_error()
    assert counts[0] > 0 and counts[4] == 0, report.value.decode()  # (ops, conflicts, ordered, ordered_reduce, races)
    # (1 + 2 + 3) / 2 = 3 exactly on the wire, / 3, x 2
    assert all((g == 2.0).all() for row in got for g in row)


def test_seventeen_ranks_are_refused(lib, gpu):
    xs = [[np.ones(300, np.float32)] for _ in range(17)]
    _thread_run(lib, gpu, 17, xs, [OP_SUM], status=INVALID_ARGUMENT)
    assert b'16' in lib.ddl_last_error()
    got, _, _, _ = _thread_run(lib, gpu, 16, xs[:16], [OP_SUM])  # the world of 16 works
    assert all((row[0] == 16.0).all() for row in got)


@pytest.fixture(scope='module')
def world(gpu):
    from ddl.torch.communicator import Communicator
    return Communicator.world()


def test_size_one_world(world, lib):
    """The keyed handler at P = 1. With the shortcut nothing is quantized; with one_rank_shortcut 0 the data plane
    runs: one quantization (no fold), also for a request cut by 64 KiB plans, out != in."""
    from ddl.torch import cpp_backend as cb
    from ddl.torch.compression import Compression
    from ddl.torch.tensor_communicate import allreduce_async, allreduce_async_batch
    x = q8.rank_input(70_001, 21)
    y = q8.rank_input(4099, 22, specials=False)
    with config(lib, one_rank_shortcut=1):
        out = allreduce_async(torch.from_numpy(x).cuda(), 'q8_short', world, compression=Compression.fp8).wait(60)
        assert out.cpu().numpy().tobytes() == x.tobytes()
    with config(lib, one_rank_shortcut=0, fusion_pipeline_bytes=0):
        with config(lib, fusion_threshold_bytes=64 << 10):  # 256 granules per plan: the request spans two plans
            src = torch.from_numpy(x).cuda()
            h = allreduce_async(src, 'q8_cut', world, compression=Compression.fp8, op=cb.OP_AVG, prescale=THIRD,
                                postscale=3.0, sumsq=True)
            out = h.wait(60)
        assert out.data_ptr() != src.data_ptr() and src.cpu().numpy().tobytes() == x.tobytes()
        want = q8.allreduce([x], OP_AVG, THIRD, 3.0)
        assert_same(DT_FLOAT, out.cpu().numpy(), want, 'request cut by 64 KiB plans')
        assert math.isnan(h.sumsq)  # the input holds NaNs
        # a batch mixing fp8 requests with what compression does not apply to, in place, with the statistic
        ts = [torch.from_numpy(y).cuda(), torch.ones(300, dtype=torch.float16, device='cuda'), torch.from_numpy(y[:253].copy()).cuda()]
        hs = allreduce_async_batch(ts, ['q8_b0', 'q8_b1', 'q8_b2'], world, outputs=ts, compression=Compression.fp8,
                                   sumsq=[True, False, True])
        for h in hs:
            h.wait(60)
        for t, v, h in ((ts[0], y, hs[0]), (ts[2], y[:253], hs[2])):
            want = q8.allreduce([v])
            assert t.cpu().numpy().tobytes() == want.tobytes()
            assert _bits(h.sumsq) == _bits(mirror(want, False))
        assert (ts[1] == 1).all()
        with config(lib, fusion_pipeline_bytes=4096):  # the same request through sub-plans: the same bits
            out = allreduce_async(torch.from_numpy(y).cuda(), 'q8_pipe', world, compression=Compression.fp8).wait(60)
        assert out.cpu().numpy().tobytes() == q8.allreduce([y]).tobytes()


def test_refusals(world, lib):
    """Every refusal of the contract, before anything is registered; a plain request works afterwards."""
    from ddl.torch import Compression, cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async
    done = cb.DONE_FN(lambda status, user: None)
    f32 = torch.ones(16, device='cuda')
    i32 = torch.ones(16, dtype=torch.int32, device='cuda')
    f16 = torch.ones(16, dtype=torch.float16, device='cuda')
    h32 = torch.ones(16)
    Q = q8.WIRE_E4M3

    def submit(t, dt, op, mem):
        return lib.ddl_allreduce_submit_mem(world.id, b'q8_refused', t.data_ptr(), t.data_ptr(), 16, dt, op, mem, _stream(),
                                            done, None)

    def submit_batch(t, dt, op, mem):
        one = (ctypes.c_void_p * 1)(t.data_ptr())
        return lib.ddl_allreduce_submit_batch_mem(world.id, 1, (ctypes.c_char_p * 1)(b'q8_refused'), one, one,
                                                  (ctypes.c_size_t * 1)(16), (ctypes.c_int * 1)(dt), op, mem, _stream(), done,
                                                  None)
    for fn in (submit, submit_batch):
        for other in (cb.WIRE_FP16, cb.WIRE_BF16, cb.WIRE_FEEDBACK, cb.WIRE_STOCHASTIC, cb.WIRE_BF16 | cb.WIRE_FEEDBACK,
                      cb.WIRE_BF16 | cb.WIRE_STOCHASTIC):
            assert fn(f32, DT_FLOAT, OP_SUM | Q | other, cb.MEMORY_DEVICE) == INVALID_ARGUMENT, hex(other)
            assert lib.ddl_last_error()
        assert fn(f32, DT_FLOAT, OP_MIN | Q, cb.MEMORY_DEVICE) == INVALID_ARGUMENT
        assert fn(f32, DT_FLOAT, OP_MAX | Q, cb.MEMORY_DEVICE) == INVALID_ARGUMENT
        assert fn(f32, DT_FLOAT, 2 | Q, cb.MEMORY_DEVICE) == INVALID_ARGUMENT
        assert fn(h32, DT_FLOAT, OP_SUM | Q, cb.MEMORY_HOST) == INVALID_ARGUMENT
        assert fn(i32, DT_INT32, OP_SUM | Q, cb.MEMORY_DEVICE) == UNSUPPORTED_DTYPE
        assert fn(f16, DT_HALF, OP_AVG | Q, cb.MEMORY_DEVICE) == UNSUPPORTED_DTYPE
    # the unkeyed entry points
    assert lib.ddl_allreduce(world.id, f32.data_ptr(), f32.data_ptr(), 16, DT_FLOAT, OP_SUM | Q, _stream()) == INVALID_ARGUMENT
    one = (ctypes.c_void_p * 1)(f32.data_ptr())
    assert lib.ddl_allreduce_batch(world.id, 1, one, one, (ctypes.c_size_t * 1)(16), DT_FLOAT, OP_SUM | Q,
                                   _stream()) == INVALID_ARGUMENT
    assert lib.ddl_allreduce_host(world.id, h32.data_ptr(), h32.data_ptr(), 16, DT_FLOAT, OP_SUM | Q) == INVALID_ARGUMENT
    # the engine's internal granule dtype is no ddl_dtype
    assert lib.ddl_dtype_size(0x1e43) == 0
    assert lib.ddl_allreduce(world.id, f32.data_ptr(), f32.data_ptr(), 0, 0x1e43, OP_SUM, _stream()) == UNSUPPORTED_DTYPE
    assert submit(f32, 0x1e43, OP_SUM, cb.MEMORY_DEVICE) == UNSUPPORTED_DTYPE
    with pytest.raises(ValueError):
        allreduce_async(f32, 'q8_minmax', world, op=cb.OP_MAX, compression=Compression.fp8)
    assert lib.ddl_wait_all(world.id) == 0
    assert torch.equal(f32.cpu(), torch.ones(16)) and torch.equal(h32, torch.ones(16))  # nothing ran
    x = torch.randn(1000, device='cuda')
    assert torch.equal(allreduce_async(x, 'q8_after_refusals', world).wait(60), x)
