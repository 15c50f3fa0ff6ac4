"""DDL_ALLREDUCE_OP_AVG through the engine on one GPU: the production RingExecutor of every
virtual rank (thread world) with the op, the batch form, the keyed fusion pipeline with per-segment
ops, the size-1 world and the refusals.

Expected values: the oracle's sum in MPICH's order (Oracle.fold_ref_order), divided on the CPU
(_avg_helpers.quotient) — bit for bit on every virtual rank."""
import ctypes

import pytest
import torch

from _avg_helpers import OP_AVG, assert_same, quotient, to_dev, to_host
from _helpers import DT_FLOAT, DT_HALF, DT_INT32, DT_INT64, DT_UINT64, NAME, config, random_input

pytestmark = pytest.mark.gpu
INVALID_ARGUMENT, UNSUPPORTED_DTYPE = 3, 4
SIZES = (1, 7, 1000, 70_001)


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope='module')
def cases(oracle):
    """(P, dtype, n) -> (rank inputs, oracle sum / P): computed once, shared, never written to."""
    out = {}
    for P in (2, 3, 5, 8):
        for dt in (DT_FLOAT, DT_HALF):
            for n in SIZES:
                xs = [random_input(dt, n, 77 * P + 1000 * dt + 13 * q + n) for q in range(P)]
                want = quotient(dt, oracle.fold_ref_order(dt, xs), P)
                want.setflags(write=False)
                out[P, dt, n] = (xs, want)
    return out


@pytest.mark.parametrize('algo', [0, 1, 2, 3, 4])
@pytest.mark.parametrize('P', [2, 3, 5, 8])
def test_thread_world_avg(lib, gpu, cases, P, algo):
    """ddl_testing_thread_allreduce_op with AVG: every schedule, out of place and in place."""
    with config(lib, algo=algo, reference_order=1, tune=0):
        for dt in (DT_FLOAT, DT_HALF):
            for n in SIZES:
                xs, want = cases[P, dt, n]
                for in_place in (False, True):
                    ins = [to_dev(x, gpu) for x in xs]
                    outs = ins if in_place else [torch.zeros_like(t) for t in ins]
                    send = (ctypes.c_void_p * P)(*[t.data_ptr() for t in ins])
                    recv = (ctypes.c_void_p * P)(*[t.data_ptr() for t in outs])
                    st = lib.ddl_testing_thread_allreduce_op(P, send, recv, n, dt, OP_AVG, _stream())
                    assert st == 0, lib.ddl_last_error()
                    torch.cuda.synchronize()
                    for r, o in enumerate(outs):
                        assert_same(dt, to_host(o, dt), want, f'{NAME[dt]} n={n} in_place={in_place} rank {r}')


@pytest.mark.parametrize('P', [2, 3, 5, 8])
@pytest.mark.parametrize('dt', [DT_FLOAT, DT_HALF], ids=lambda d: NAME[d])
def test_thread_world_avg_batch(lib, oracle, gpu, P, dt):
    """The grouped form: 5 buckets in one program, one dividing launch over all of them."""
    elems = [1, 300, 4099, 70_001, 513]
    k = len(elems)
    xs = [[random_input(dt, n, 5 * P + 31 * q + b) for b, n in enumerate(elems)] for q in range(P)]
    wants = [quotient(dt, oracle.fold_ref_order(dt, [xs[q][b] for q in range(P)]), P) for b in range(k)]
    bufs = [[to_dev(x, gpu) for x in row] for row in xs]
    ptrs = (ctypes.c_void_p * (P * k))(*[t.data_ptr() for row in bufs for t in row])
    with config(lib, reference_order=1, tune=0):
        st = lib.ddl_testing_thread_allreduce_batch_op(P, k, ptrs, ptrs, (ctypes.c_size_t * k)(*elems), dt, OP_AVG,
                                                       _stream())
        assert st == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    for r in range(P):
        for b in range(k):
            assert_same(dt, to_host(bufs[r][b], dt), wants[b], f'rank {r} bucket {b}')


@pytest.mark.parametrize('P', [3, 5])
def test_thread_world_fused_mixed_ops(lib, oracle, gpu, P):
    """The keyed path's FusionPipe with per-segment ops, cut into 256 KiB sub-plans (segments are
    split across sub-plans): every segment is the oracle's sum for the plan's message size, divided
    where its op is AVG — SUM and AVG segments share plans, sub-plans and unpack launches."""
    dt, elems = DT_FLOAT, [5, 300, 70_001, 4099, 1, 200_000, 513]
    k = len(elems)
    ops = [i % 2 for i in range(k)]  # SUM, AVG, SUM, ...
    message = 4 * sum(elems)
    xs = [[random_input(dt, n, 900 + 17 * q + i) for i, n in enumerate(elems)] for q in range(P)]
    ins = [[to_dev(x, gpu) for x in row] for row in xs]
    outs = [[torch.zeros_like(t) for t in row] for row in ins]
    S = (ctypes.c_void_p * (P * k))(*[t.data_ptr() for row in ins for t in row])
    D = (ctypes.c_void_p * (P * k))(*[t.data_ptr() for row in outs for t in row])
    J = ctypes.c_size_t()
    with config(lib, reference_order=1, tune=0, fusion_pipeline_bytes=256 << 10):
        st = lib.ddl_testing_thread_fused_allreduce_ops(P, k, S, D, (ctypes.c_size_t * k)(*[4 * n for n in elems]),
                                                        (ctypes.c_int * k)(*ops), dt, _stream(), ctypes.byref(J))
        assert st == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    assert J.value > 1
    for i in range(k):
        total = oracle.fold_ref_order(dt, [xs[q][i] for q in range(P)], message)
        want = quotient(dt, total, P) if ops[i] == OP_AVG else total
        for r in range(P):
            assert_same(dt, to_host(outs[r][i], dt), want, f'segment {i} op {ops[i]} rank {r}')


@pytest.mark.parametrize('P', [3, 5])
def test_local_world_avg(lib, gpu, cases, P):
    """ddl_local_ring_allreduce accepts AVG: the device-copy world's results, divided by one launch."""
    for n in (7, 70_001):
        xs, want = cases[P, DT_FLOAT, n]
        ins = [to_dev(x, gpu) for x in xs]
        outs = [torch.zeros_like(t) for t in ins]
        send = (ctypes.c_void_p * P)(*[t.data_ptr() for t in ins])
        recv = (ctypes.c_void_p * P)(*[t.data_ptr() for t in outs])
        with config(lib, reference_order=1, tune=0):
            assert lib.ddl_local_ring_allreduce(P, send, recv, n, DT_FLOAT, OP_AVG, _stream()) == 0, lib.ddl_last_error()
        torch.cuda.synchronize()
        for r, o in enumerate(outs):
            assert_same(DT_FLOAT, to_host(o, DT_FLOAT), want, f'n={n} rank {r}')
    assert lib.ddl_local_ring_allreduce(P, send, recv, n, DT_INT32, OP_AVG, _stream()) == UNSUPPORTED_DTYPE
    assert lib.ddl_local_ring_allreduce(P, send, recv, n, DT_FLOAT, 2, _stream()) == INVALID_ARGUMENT


@pytest.fixture(scope='module')
def world(gpu):
    from ddl.torch.communicator import Communicator
    return Communicator.world()


@pytest.mark.parametrize('shortcut', [0, 1])
def test_size_one_world_avg_is_the_input(world, lib, shortcut):
    """P = 1: AVG is SUM, which is the input — keyed (fused and single plans, device and host) and
    direct, bit for bit."""
    from ddl.torch import cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce, allreduce_async_batch
    ts = [torch.randn(n, device='cuda').to(d) for n, d in ((5, torch.float32), (70_001, torch.float32),
                                                            (333, torch.float16), (4099, torch.bfloat16),
                                                            (1000, torch.float64))]
    ts += [torch.randn(4099), torch.randn(257).pin_memory()]
    with config(lib, one_rank_shortcut=shortcut):
        hs = allreduce_async_batch(ts, [f'avg1_{shortcut}_{i:03d}' for i in range(len(ts))], world, op=cb.OP_AVG)
        for t, h in zip(ts, hs):
            assert torch.equal(h.wait(60).view(torch.uint8), t.view(torch.uint8))
        assert torch.equal(allreduce(ts[1], world, op=cb.OP_AVG), ts[1])
        assert torch.equal(allreduce(ts[5], world, op=cb.OP_AVG), ts[5])


def test_refusals(world, lib):
    """AVG on an integer dtype: UNSUPPORTED_DTYPE from every entry point; an unknown op:
    INVALID_ARGUMENT; nothing is posted, and the communicator works afterwards."""
    from ddl.torch import cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce
    done = cb.DONE_FN(lambda status, user: None)
    for dt, tdt in ((DT_INT32, torch.int32), (DT_INT64, torch.int64), (DT_UINT64, torch.int64), (DT_FLOAT, torch.float32)):
        op, want = (2, INVALID_ARGUMENT) if dt == DT_FLOAT else (OP_AVG, UNSUPPORTED_DTYPE)
        d, h = torch.ones(16, dtype=tdt, device='cuda'), torch.ones(16, dtype=tdt)
        one = (ctypes.c_void_p * 1)(d.data_ptr())
        hone = (ctypes.c_void_p * 1)(h.data_ptr())
        n1, dts = (ctypes.c_size_t * 1)(16), (ctypes.c_int * 1)(dt)
        keys = (ctypes.c_char_p * 1)(b'refused')
        users = (ctypes.c_void_p * 1)(None)
        assert lib.ddl_allreduce(world.id, d.data_ptr(), d.data_ptr(), 16, dt, op, _stream()) == want
        assert lib.ddl_allreduce_batch(world.id, 1, one, one, n1, dt, op, _stream()) == want
        assert lib.ddl_allreduce_host(world.id, h.data_ptr(), h.data_ptr(), 16, dt, op) == want
        for mem, p, arr in ((cb.MEMORY_DEVICE, d.data_ptr(), one), (cb.MEMORY_HOST, h.data_ptr(), hone)):
            assert lib.ddl_allreduce_submit_mem(world.id, b'refused', p, p, 16, dt, op, mem, _stream(), done, None) == want
            assert lib.ddl_allreduce_submit_batch_mem(world.id, 1, keys, arr, arr, n1, dts, op, mem, _stream(), done,
                                                      users) == want
        assert lib.ddl_last_error()
    assert lib.ddl_wait_all(world.id) == 0  # nothing was registered
    x = torch.randn(100, device='cuda')
    assert torch.equal(allreduce(x, world), x) and torch.equal(allreduce(x, world, op=cb.OP_AVG), x)
