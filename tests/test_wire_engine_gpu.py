"""Wire compression through the engine on one GPU: the compressed fusion plan of every virtual rank
(thread world: converting pack, allreduce in the wire dtype, converting unpack with per-segment
ops), the size-1 world through the Python API, and the refusals.

Expected values (_wire_helpers.expected): each rank's input cast on the CPU, the oracle's sum of
the casts in MPICH's order for the plan's unpadded wire bytes, widened, divided by np.float32(P)
where the op is AVG — bit for bit on every virtual rank."""
import ctypes

import pytest
import torch

from _avg_helpers import assert_same, to_dev, to_host
from _helpers import DT_BFLOAT16, DT_DOUBLE, DT_FLOAT, DT_HALF, DT_INT32, config
from _wire_helpers import (OP_AVG, OP_SUM, WIRE_BF16, WIRE_DT, WIRE_FP16, WIRE_NAME, WIRES, expected, narrow, widen,
                           wire_input)

pytestmark = pytest.mark.gpu
INVALID_ARGUMENT, UNSUPPORTED_DTYPE = 3, 4
ELEMENTS = [5, 300, 70_001, 4099, 1, 200_000, 513]


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope='module')
def inputs():
    """P -> the ranks' fp32 segments: computed once, shared, never written to."""
    out = {}
    for P in (2, 3, 5, 8):
        out[P] = [[wire_input(n, 1300 + 101 * P + 17 * q + i) for i, n in enumerate(ELEMENTS)] for q in range(P)]
        for row in out[P]:
            for x in row:
                x.setflags(write=False)
    return out


def _run(lib, gpu, P, rows, elems, ops, wire):
    k = len(elems)
    ins = [[to_dev(x.copy(), gpu) for x in row] for row in rows]  # (the shared inputs are read-only)
    outs = [[torch.zeros_like(t) for t in row] for row in ins]
    S = (ctypes.c_void_p * (P * k))(*[t.data_ptr() for row in ins for t in row])
    D = (ctypes.c_void_p * (P * k))(*[t.data_ptr() for row in outs for t in row])
    J = ctypes.c_size_t()
    st = lib.ddl_testing_thread_fused_allreduce_wire(P, k, S, D, (ctypes.c_size_t * k)(*elems), (ctypes.c_int * k)(*ops),
                                                     wire, _stream(), ctypes.byref(J))
    assert st == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    return outs, J.value


@pytest.mark.parametrize('pipeline', [0, 256 << 10], ids=['unpipelined', 'pipelined'])
@pytest.mark.parametrize('wire', WIRES, ids=lambda d: WIRE_NAME[d])
@pytest.mark.parametrize('P', [2, 3, 5, 8])
def test_thread_world_compressed_plan(lib, oracle, gpu, inputs, P, wire, pipeline):
    """Seven fp32 segments with alternating SUM / AVG over a 16-bit wire, as one plan and cut into
    256 KiB sub-plans of the wire stream (segments split across sub-plans)."""
    rows, k = inputs[P], len(ELEMENTS)
    ops = [i % 2 for i in range(k)]  # SUM, AVG, SUM, ...
    message = 2 * sum(ELEMENTS)      # the plan's unpadded wire bytes
    with config(lib, reference_order=1, tune=0, fusion_pipeline_bytes=pipeline):
        outs, J = _run(lib, gpu, P, rows, ELEMENTS, ops, wire)
    assert (J > 1) if pipeline else (J == 1)
    for i in range(k):
        want = expected(oracle, wire, [rows[q][i] for q in range(P)], message, ops[i], P)
        for r in range(P):
            assert_same(DT_FLOAT, to_host(outs[r][i], DT_FLOAT), want,
                        f'{WIRE_NAME[wire]} P={P} segment {i} op {ops[i]} rank {r}')


@pytest.mark.parametrize('wire', WIRES, ids=lambda d: WIRE_NAME[d])
def test_thread_world_one_request_plan(lib, oracle, gpu, inputs, wire):
    """A compressed plan of one request still goes through the fusion buffer (there is no in-place
    path for it): one 4099-element AVG segment at P = 3."""
    P, i = 3, ELEMENTS.index(4099)
    rows = [[inputs[P][q][i]] for q in range(P)]
    with config(lib, reference_order=1, tune=0, fusion_pipeline_bytes=0):
        outs, J = _run(lib, gpu, P, rows, [4099], [OP_AVG], wire)
    want = expected(oracle, wire, [r[0] for r in rows], 2 * 4099, OP_AVG, P)
    for r in range(P):
        assert_same(DT_FLOAT, to_host(outs[r][0], DT_FLOAT), want, f'{WIRE_NAME[wire]} rank {r}')


@pytest.fixture(scope='module')
def world(gpu):
    from ddl.torch.communicator import Communicator
    return Communicator.world()


@pytest.mark.parametrize('flag', [WIRE_FP16, WIRE_BF16], ids=['fp16', 'bf16'])
@pytest.mark.parametrize('shortcut', [1, 0])
def test_size_one_world(world, lib, gpu, shortcut, flag):
    """P = 1 through the Python API. one_rank_shortcut 1: nothing is communicated and nothing is
    compressed — the input, bit for bit. 0: the data plane runs — the input round-tripped through
    the wire type (fused plans and a one-request plan, SUM and AVG: at P = 1 the quotient is the
    value). Tensors that are not fp32 device tensors come back as they were either way."""
    from ddl.torch import Compression, cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async, allreduce_async_batch
    comp = Compression.fp16 if flag == WIRE_FP16 else Compression.bf16
    wire = WIRE_DT[flag]
    xs = [wire_input(n, 50 + n) for n in (5, 70_001, 513)]
    ts = [to_dev(x, gpu) for x in xs] + [torch.randn(333, device='cuda').half(), torch.randn(257)]
    with config(lib, one_rank_shortcut=shortcut):
        for op in (cb.OP_SUM, cb.OP_AVG):
            names = [f'wire1_{shortcut}_{flag}_{op}_{i:03d}' for i in range(len(ts))]
            hs = allreduce_async_batch(ts, names, world, op=op, compression=comp)
            for i, (t, h) in enumerate(zip(ts, hs)):
                got = h.wait(60)
                if i < len(xs) and shortcut == 0:
                    assert_same(DT_FLOAT, to_host(got, DT_FLOAT), widen(wire, narrow(wire, xs[i])), f'tensor {i}')
                else:
                    assert torch.equal(got.view(torch.uint8), t.view(torch.uint8)), f'tensor {i}'
        got = allreduce_async(ts[1], f'wire1_single_{shortcut}_{flag}', world, compression=comp).wait(60)
        want = widen(wire, narrow(wire, xs[1])) if shortcut == 0 else xs[1]
        assert_same(DT_FLOAT, to_host(got, DT_FLOAT), want, 'one-request plan')


def test_refusals(world, lib, gpu):
    """Every refusal of the contract, before anything is registered; the communicator works
    afterwards."""
    from ddl.torch import cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce
    done = cb.DONE_FN(lambda status, user: None)
    n = 16
    f32, f32h = torch.ones(n, device='cuda'), torch.ones(n)
    keys, users, n1 = (ctypes.c_char_p * 1)(b'refused'), (ctypes.c_void_p * 1)(None), (ctypes.c_size_t * 1)(n)

    def submit(t, dt, op, mem):
        p = t.data_ptr()
        one = (ctypes.c_void_p * 1)(p)
        return (lib.ddl_allreduce_submit_mem(world.id, b'refused', p, p, n, dt, op, mem, _stream(), done, None),
                lib.ddl_allreduce_submit_batch_mem(world.id, 1, keys, one, one, n1, (ctypes.c_int * 1)(dt), op, mem,
                                                   _stream(), done, users))

    for flag in (WIRE_FP16, WIRE_BF16):
        for op in (OP_SUM | flag, OP_AVG | flag):
            # a wire flag on any dtype but fp32
            for dt, tdt in ((DT_HALF, torch.float16), (DT_BFLOAT16, torch.bfloat16), (DT_DOUBLE, torch.float64),
                            (DT_INT32, torch.int32)):
                assert submit(torch.ones(n, dtype=tdt, device='cuda'), dt, op, cb.MEMORY_DEVICE) == \
                    (UNSUPPORTED_DTYPE,) * 2, (op, dt)
            # host memory
            assert submit(f32h, DT_FLOAT, op, cb.MEMORY_HOST) == (INVALID_ARGUMENT,) * 2
            # the unkeyed entry points
            p, one = f32.data_ptr(), (ctypes.c_void_p * 1)(f32.data_ptr())
            assert lib.ddl_allreduce(world.id, p, p, n, DT_FLOAT, op, _stream()) == INVALID_ARGUMENT
            assert lib.ddl_allreduce_batch(world.id, 1, one, one, n1, DT_FLOAT, op, _stream()) == INVALID_ARGUMENT
            assert lib.ddl_allreduce_host(world.id, f32h.data_ptr(), f32h.data_ptr(), n, DT_FLOAT, op) == INVALID_ARGUMENT
    # both flags, and unknown bits with and without a flag
    for op in (WIRE_FP16 | WIRE_BF16, WIRE_FP16 | WIRE_BF16 | OP_AVG, 0x400, 0x400 | WIRE_FP16, 2 | WIRE_BF16, 0x80, -1):
        assert submit(f32, DT_FLOAT, op, cb.MEMORY_DEVICE) == (INVALID_ARGUMENT,) * 2, hex(op)
    # a batch is all-or-nothing: one fp16 entry among fp32 ones fails it, and registers nothing
    ts = [torch.ones(n, device='cuda'), torch.ones(n, device='cuda').half(), torch.ones(n, device='cuda')]
    ptrs = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in ts])
    st = lib.ddl_allreduce_submit_batch_mem(world.id, 3, (ctypes.c_char_p * 3)(b'mix_a', b'mix_b', b'mix_c'), ptrs, ptrs,
                                            (ctypes.c_size_t * 3)(n, n, n), (ctypes.c_int * 3)(DT_FLOAT, DT_HALF, DT_FLOAT),
                                            OP_SUM | WIRE_FP16, cb.MEMORY_DEVICE, _stream(), done,
                                            (ctypes.c_void_p * 3)(None, None, None))
    assert st == UNSUPPORTED_DTYPE and lib.ddl_last_error()
    assert lib.ddl_wait_all(world.id) == 0  # nothing was registered
    x = torch.randn(100, device='cuda')
    assert torch.equal(allreduce(x, world), x)
