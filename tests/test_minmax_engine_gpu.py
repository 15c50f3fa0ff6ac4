"""DDL_ALLREDUCE_OP_MIN / _MAX through the engine on one GPU: every schedule of the device-copy
world, the production RingExecutor of every virtual rank (thread world) with the happens-before
recorder on, the keyed fusion pipeline, the one-rank world, the refusals and a hipGraph capture.

Expected values: the numpy model of tests/_minmax_helpers.py — the operation is associative and
commutative, so one model covers every schedule, order and P. Every rank, bit for bit."""
import ctypes

import pytest
import torch

from _avg_helpers import to_dev, to_host
from _helpers import ALL_DTYPES, DT_FLOAT, DT_HALF, DT_INT32, NAME, config
from _minmax_helpers import OP_MAX, OP_MIN, OP_NAME, OPS, assert_same, finite_input, model

pytestmark = pytest.mark.gpu
INVALID_ARGUMENT = 3
VP, SZ = ctypes.c_void_p, ctypes.c_size_t
BY_OP = dict(ids=lambda o: OP_NAME[o])
SIZES = (7, 70_001)  # both sides of the 2048-byte order switch
WIRE_FP16, WIRE_BF16, WIRE_FEEDBACK = 0x100, 0x200, 0x1000


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope='module')
def cases():
    """(P, dtype, n) -> (rank inputs, {op: model}): computed once, shared, never written to."""
    cache = {}

    def get(P, dt, n):
        if (P, dt, n) not in cache:
            xs = [finite_input(dt, n, 77 * P + 1000 * dt + 13 * q + n) for q in range(P)]
            want = {op: model(dt, op, xs) for op in OPS}
            for w in want.values():
                w.setflags(write=False)
            cache[P, dt, n] = (xs, want)
        return cache[P, dt, n]
    return get


def _local(lib, gpu, cases, P, dt, n, op, in_place):
    xs, want = cases(P, dt, n)
    ins = [to_dev(x, gpu) for x in xs]
    outs = ins if in_place else [torch.zeros_like(t) for t in ins]
    send = (VP * P)(*[t.data_ptr() for t in ins])
    recv = (VP * P)(*[t.data_ptr() for t in outs])
    assert lib.ddl_local_ring_allreduce(P, send, recv, n, dt, op, _stream()) == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    for r, o in enumerate(outs):
        assert_same(dt, to_host(o, dt), want[op], f'{NAME[dt]} P={P} n={n} {OP_NAME[op]} in_place={in_place} rank {r}')


@pytest.mark.parametrize('ref', [0, 1])
@pytest.mark.parametrize('algo', [0, 1, 2, 3, 4])
@pytest.mark.parametrize('P', [2, 3, 5, 8, 17, 33])
def test_local_world_every_schedule(lib, gpu, cases, P, algo, ref):
    """ddl_local_ring_allreduce, fp32: every schedule, with and without the reference order (which
    MIN / MAX do not depend on), partial folds beyond 16 ranks, in place and out of place."""
    with config(lib, algo=algo, reference_order=ref, tune=0):
        for n in SIZES:
            for op in OPS:
                _local(lib, gpu, cases, P, DT_FLOAT, n, op, in_place=(op == OP_MAX))
                _local(lib, gpu, cases, P, DT_FLOAT, n, op, in_place=(op == OP_MIN))


@pytest.mark.parametrize('dt', [d for d in ALL_DTYPES if d != DT_FLOAT], ids=lambda d: NAME[d])
def test_local_world_every_dtype(lib, gpu, cases, dt):
    """Every other dtype at P = 5 direct (algo 1) and P = 2 ring (algo 0)."""
    for P, algo in ((5, 1), (2, 0)):
        with config(lib, algo=algo, reference_order=1, tune=0):
            for n in SIZES:
                for op in OPS:
                    _local(lib, gpu, cases, P, dt, n, op, in_place=False)
                    _local(lib, gpu, cases, P, dt, n, op, in_place=True)


def _traced(lib, fn):
    assert lib.ddl_testing_dep_trace(1) == 0, lib.ddl_last_error()
    try:
        fn()
    finally:
        assert lib.ddl_testing_dep_trace(0) == 0, lib.ddl_last_error()
    counts = (ctypes.c_longlong * 5)()
    buf = ctypes.create_string_buffer(1 << 14)
    assert lib.ddl_testing_dep_check(counts, buf, len(buf)) == 0, lib.ddl_last_error()
    return dict(zip(('ops', 'conflicts', 'ordered', 'ordered_reduce', 'races'), counts)), buf.value.decode()


@pytest.mark.parametrize('op', OPS, **BY_OP)
@pytest.mark.parametrize('P', [5, 8])
def test_thread_world_op_and_batch(lib, gpu, cases, P, op):
    """The production executor per rank (ddl_testing_thread_allreduce_op / _batch_op) with the
    happens-before recorder on: no race, and every rank equals the model."""
    with config(lib, reference_order=1, tune=0):
        for dt in (DT_FLOAT, DT_HALF):
            for n in SIZES:
                xs, want = cases(P, dt, n)
                ins = [to_dev(x, gpu) for x in xs]
                outs = [torch.zeros_like(t) for t in ins]
                send = (VP * P)(*[t.data_ptr() for t in ins])
                recv = (VP * P)(*[t.data_ptr() for t in outs])
                res, lines = _traced(lib, lambda: _check(lib, lib.ddl_testing_thread_allreduce_op(
                    P, send, recv, n, dt, op, _stream())))
                torch.cuda.synchronize()
                assert res['races'] == 0 and res['ops'] > 0, lines
                for r, o in enumerate(outs):
                    assert_same(dt, to_host(o, dt), want[op], f'{NAME[dt]} n={n} rank {r}')
        dt, elems = DT_FLOAT, [1, 300, 4099, 70_001, 513]
        k = len(elems)
        xs = [[finite_input(dt, n, 5 * P + 31 * q + b) for b, n in enumerate(elems)] for q in range(P)]
        bufs = [[to_dev(x, gpu) for x in row] for row in xs]
        ptrs = (VP * (P * k))(*[t.data_ptr() for row in bufs for t in row])
        res, lines = _traced(lib, lambda: _check(lib, lib.ddl_testing_thread_allreduce_batch_op(
            P, k, ptrs, ptrs, (SZ * k)(*elems), dt, op, _stream())))
        torch.cuda.synchronize()
        assert res['races'] == 0 and res['ops'] > 0, lines
        for b in range(k):
            want = model(dt, op, [xs[q][b] for q in range(P)])
            for r in range(P):
                assert_same(dt, to_host(bufs[r][b], dt), want, f'rank {r} bucket {b}')


def _check(lib, st):
    assert st == 0, lib.ddl_last_error()


@pytest.mark.parametrize('op', OPS, **BY_OP)
@pytest.mark.parametrize('P', [3, 5])
def test_thread_world_fused_plan(lib, gpu, P, op):
    """The keyed path's FusionPipe with every segment of one kind, cut into 256 KiB sub-plans
    (at least 3; segments are split across them): pack -> allreduce(kind) -> plain unpack. A plan
    that mixes kinds is refused."""
    dt, elems = DT_FLOAT, [5, 300, 70_001, 4099, 1, 200_000, 513]
    k = len(elems)
    xs = [[finite_input(dt, n, 900 + 17 * q + i) for i, n in enumerate(elems)] for q in range(P)]
    ins = [[to_dev(x, gpu) for x in row] for row in xs]
    outs = [[torch.zeros_like(t) for t in row] for row in ins]
    S = (VP * (P * k))(*[t.data_ptr() for row in ins for t in row])
    D = (VP * (P * k))(*[t.data_ptr() for row in outs for t in row])
    B = (SZ * k)(*[4 * n for n in elems])
    J = SZ()
    with config(lib, reference_order=1, tune=0, fusion_pipeline_bytes=256 << 10):
        st = lib.ddl_testing_thread_fused_allreduce_ops(P, k, S, D, B, (ctypes.c_int * k)(*([op] * k)), dt, _stream(),
                                                        ctypes.byref(J))
        assert st == 0, lib.ddl_last_error()
        torch.cuda.synchronize()
        assert J.value >= 3
        for other in (0, 1, OP_MIN if op == OP_MAX else OP_MAX):
            mixed = (ctypes.c_int * k)(*([op] * (k - 1) + [other]))
            assert lib.ddl_testing_thread_fused_allreduce_ops(P, k, S, D, B, mixed, dt, _stream(),
                                                              None) == INVALID_ARGUMENT
    torch.cuda.synchronize()
    for i in range(k):
        want = model(dt, op, [xs[q][i] for q in range(P)])
        for r in range(P):
            assert_same(dt, to_host(outs[r][i], dt), want, f'segment {i} rank {r}')
            assert to_host(ins[r][i], dt).tobytes() == xs[r][i].tobytes()


@pytest.fixture(scope='module')
def world(gpu):
    from ddl.torch.communicator import Communicator
    return Communicator.world()


@pytest.mark.parametrize('shortcut', [0, 1])
def test_one_rank_world_is_the_input(world, lib, shortcut):
    """P = 1: the result is the input, bit for bit (NaNs and signed zeros included) — keyed (fused and
    single plans, device and host, MIN and MAX in one round) and direct, with and without the
    one-rank shortcut."""
    from ddl.torch import cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce, allreduce_async_batch
    ts = [torch.randn(n, device='cuda').to(d) for n, d in ((5, torch.float32), (70_001, torch.float32),
                                                            (333, torch.float16), (4099, torch.bfloat16),
                                                            (1000, torch.float64))]
    ts[0][:3] = torch.tensor([float('nan'), -0.0, float('inf')], device='cuda')
    ts += [torch.randint(-1000, 1000, (513,), device='cuda', dtype=torch.int32), torch.randn(4099),
           torch.randn(257).pin_memory()]
    with config(lib, one_rank_shortcut=shortcut):
        for op in (cb.OP_MIN, cb.OP_MAX):
            hs = allreduce_async_batch(ts, [f'mm1_{shortcut}_{op}_{i:03d}' for i in range(len(ts))], world, op=op)
            for t, h in zip(ts, hs):
                assert torch.equal(h.wait(60).view(torch.uint8), t.view(torch.uint8))
            for t in (ts[1], ts[5], ts[6]):
                assert torch.equal(allreduce(t, world, op=op).view(torch.uint8), t.view(torch.uint8))


def test_refusals(world, lib):
    """MIN / MAX with a wire flag or the feedback bit, and the op values 2 and 5: INVALID_ARGUMENT
    from every entry point, nothing registered, and the communicator works afterwards."""
    from ddl.torch import cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce
    done = cb.DONE_FN(lambda status, user: None)
    d, h = torch.ones(16, device='cuda'), torch.ones(16)
    one, hone = (VP * 1)(d.data_ptr()), (VP * 1)(h.data_ptr())
    n1, dts = (SZ * 1)(16), (ctypes.c_int * 1)(DT_FLOAT)
    keys, users = (ctypes.c_char_p * 1)(b'refused'), (VP * 1)(None)
    bad = [2, 5] + [m | w for m in (OP_MIN, OP_MAX) for w in (WIRE_FP16, WIRE_BF16, WIRE_FP16 | WIRE_FEEDBACK,
                                                                  WIRE_BF16 | WIRE_FEEDBACK, WIRE_FEEDBACK)]
    for op in bad:
        assert lib.ddl_allreduce(world.id, d.data_ptr(), d.data_ptr(), 16, DT_FLOAT, op, _stream()) == INVALID_ARGUMENT
        assert lib.ddl_allreduce_batch(world.id, 1, one, one, n1, DT_FLOAT, op, _stream()) == INVALID_ARGUMENT
        assert lib.ddl_allreduce_host(world.id, h.data_ptr(), h.data_ptr(), 16, DT_FLOAT, op) == INVALID_ARGUMENT
        assert lib.ddl_allreduce_variant(world.id, d.data_ptr(), d.data_ptr(), 16, DT_FLOAT, op, _stream(),
                                         0) == INVALID_ARGUMENT
        assert lib.ddl_local_ring_allreduce(1, one, one, 16, DT_FLOAT, op, _stream()) == INVALID_ARGUMENT
        assert lib.ddl_testing_thread_allreduce_op(1, one, one, 16, DT_FLOAT, op, _stream()) == INVALID_ARGUMENT
        assert lib.ddl_testing_thread_allreduce_batch_op(1, 1, one, one, n1, DT_FLOAT, op, _stream()) == INVALID_ARGUMENT
        for mem, p, arr in ((cb.MEMORY_DEVICE, d.data_ptr(), one), (cb.MEMORY_HOST, h.data_ptr(), hone)):
            assert lib.ddl_allreduce_submit_mem(world.id, b'refused', p, p, 16, DT_FLOAT, op, mem, _stream(), done,
                                                None) == INVALID_ARGUMENT, op
            assert lib.ddl_allreduce_submit_batch_mem(world.id, 1, keys, arr, arr, n1, dts, op, mem, _stream(), done,
                                                      users) == INVALID_ARGUMENT, op
        assert lib.ddl_last_error()
    assert lib.ddl_wait_all(world.id) == 0  # nothing was registered
    x = torch.randn(100, device='cuda')
    for op in (cb.OP_SUM, cb.OP_MIN, cb.OP_MAX):
        assert torch.equal(allreduce(x, world, op=op), x)
    i = torch.arange(-5, 5, device='cuda', dtype=torch.int32)
    assert torch.equal(allreduce(i, world, op=cb.OP_MAX), i)  # integers take MIN / MAX (unlike AVG)
    assert lib.ddl_allreduce_variant(world.id, x.data_ptr(), x.data_ptr(), 100, DT_FLOAT, OP_MAX, _stream(), 0) == 0
    assert lib.ddl_allreduce(world.id, i.data_ptr(), i.data_ptr(), 10, DT_INT32, OP_MIN, _stream()) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize('P,algo', [(5, 1), (2, 0)])
def test_max_allreduce_graph_replay(world, lib, gpu, P, algo):
    """A MAX allreduce captured into a hipGraph and replayed on fresh inputs: the world communicator's
    ddl_allreduce, and P virtual ranks' programs (the reduce / fold launches are the program's own, no
    trailing launch). Warmed up once outside the capture, as tests/test_graph_gpu.py does."""
    n = 70_001
    s = torch.cuda.Stream()
    ins = [torch.zeros(n, device=gpu) for _ in range(P)]
    outs = [torch.empty_like(t) for t in ins]
    a, b = torch.zeros(n, device=gpu), torch.empty(n, device=gpu)
    send = (VP * P)(*[t.data_ptr() for t in ins])
    recv = (VP * P)(*[t.data_ptr() for t in outs])

    def post():
        assert lib.ddl_allreduce(world.id, a.data_ptr(), b.data_ptr(), n, DT_FLOAT, OP_MAX, s.cuda_stream) == 0, \
            lib.ddl_last_error()
        assert lib.ddl_local_ring_allreduce(P, send, recv, n, DT_FLOAT, OP_MAX, s.cuda_stream) == 0, lib.ddl_last_error()
    with config(lib, algo=algo, reference_order=1, tune=0):
        with torch.cuda.stream(s):  # warm-up: sizes staging and events
            post()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            post()
        for rep in range(3):
            xs = [finite_input(DT_FLOAT, n, 7 + 31 * rep + 7919 * r) for r in range(P)]
            for r in range(P):
                ins[r].copy_(torch.from_numpy(xs[r]).to(gpu))
            a.copy_(ins[0])
            g.replay()
            torch.cuda.synchronize()
            want = model(DT_FLOAT, OP_MAX, xs)
            assert torch.equal(a, b)
            for r in range(P):
                assert_same(DT_FLOAT, outs[r].cpu().numpy(), want, f'replay {rep} rank {r}')
        del g
