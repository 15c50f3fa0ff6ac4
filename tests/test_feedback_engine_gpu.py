"""Error feedback of the 16-bit wire through the engine on one GPU: the compressed fusion plan of
every virtual rank with caller-owned residuals (thread world, unpipelined and cut into sub-plans),
the keyed handler's own per-key residual store through the Python API on a one-rank world, and the
refusals.

Expected values: _feedback_helpers (the rule on the CPU with numpy's / torch CPU's casts) for every
rank's wire values and residuals, then the oracle's sum of the wire values in MPICH's order for the
plan's unpadded wire bytes, widened, divided by np.float32(P) where the op is AVG — bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from _avg_helpers import assert_same, to_dev, to_host
from _feedback_helpers import WIRE_FEEDBACK, constant_sequence, reduce_ref, step_or_cast
from _helpers import DT_BFLOAT16, DT_DOUBLE, DT_FLOAT, DT_HALF, DT_INT32, config
from _wire_helpers import OP_AVG, OP_SUM, WIRE_BF16, WIRE_FP16, WIRE_NAME, WIRES, wire_input

pytestmark = pytest.mark.gpu
INVALID_ARGUMENT, UNSUPPORTED_DTYPE = 3, 4
ELEMENTS = [5, 300, 70_001, 4099, 1, 513]  # 70_001 elements = 140 KB on the wire: cut by a 64 KiB pipeline
OPS = [i % 2 for i in range(len(ELEMENTS))]  # SUM, AVG, SUM, ...
ROUNDS = 3
BF16_SEQ = [1, 1, 1, 1, 1.0078125, 1, 1, 1]  # a constant 1 + 2**-10 over bf16 from residual 0 (the issue's pin)
VALUE = 1 + 2.0 ** -10


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _no_residual(r, i):
    """Which (rank, segment) pairs run without feedback: the bit is rank-local, one launch mixes both."""
    return (r + i) % 4 == 3


@pytest.fixture(scope='module')
def model(oracle):
    """(P, wire) -> the rounds' inputs, expected outputs and expected residuals: computed once per
    pair on first use, shared by the unpipelined and the pipelined run, never written to."""
    cache = {}

    def get(P, wire):
        if (P, wire) in cache:
            return cache[P, wire]
        k, message = len(ELEMENTS), 2 * sum(ELEMENTS)
        resid = [[None if _no_residual(r, i) else np.zeros(n, np.float32) for i, n in enumerate(ELEMENTS)]
                 for r in range(P)]
        rounds = []
        for t in range(ROUNDS):
            xs = [[wire_input(n, 2300 + 1000 * t + 101 * P + 17 * r + i) for i, n in enumerate(ELEMENTS)]
                  for r in range(P)]
            stepped = [[step_or_cast(wire, xs[r][i], resid[r][i]) for i in range(k)] for r in range(P)]
            resid = [[stepped[r][i][1] for i in range(k)] for r in range(P)]
            outs = [reduce_ref(oracle, wire, [stepped[r][i][0] for r in range(P)], message, OPS[i], P) for i in range(k)]
            for a in [x for row in xs for x in row] + outs + [x for row in resid for x in row if x is not None]:
                a.setflags(write=False)
            rounds.append((xs, outs, resid))
        cache[P, wire] = rounds
        return rounds
    return get


@pytest.mark.parametrize('pipeline', [0, 64 << 10], ids=['unpipelined', 'pipelined'])
@pytest.mark.parametrize('wire', WIRES, ids=lambda d: WIRE_NAME[d])
@pytest.mark.parametrize('P', [2, 3, 8])
def test_thread_world_feedback_plan(lib, gpu, model, P, wire, pipeline):
    """Three rounds on the same residuals; every rank's output and every residual after every
    round. Pipelined, the 70_001-element segment is cut across sub-plans: its residual is taken at
    the tensor's own element offset, and no bit changes."""
    k = len(ELEMENTS)
    res = [[None if _no_residual(r, i) else torch.zeros(n, dtype=torch.float32, device=gpu)
            for i, n in enumerate(ELEMENTS)] for r in range(P)]
    R = (ctypes.c_void_p * (P * k))(*[t.data_ptr() if t is not None else None for row in res for t in row])
    with config(lib, reference_order=1, tune=0, fusion_pipeline_bytes=pipeline):
        for t, (xs, want_out, want_res) in enumerate(model(P, wire)):
            ins = [[to_dev(x.copy(), gpu) for x in row] for row in xs]
            outs = [[torch.zeros_like(x) for x in row] for row in ins]
            S = (ctypes.c_void_p * (P * k))(*[x.data_ptr() for row in ins for x in row])
            D = (ctypes.c_void_p * (P * k))(*[x.data_ptr() for row in outs for x in row])
            J = ctypes.c_size_t()
            st = lib.ddl_testing_thread_fused_allreduce_wire_fb(P, k, S, D, R, (ctypes.c_size_t * k)(*ELEMENTS),
                                                                (ctypes.c_int * k)(*OPS), wire, _stream(), ctypes.byref(J))
            assert st == 0, lib.ddl_last_error()
            torch.cuda.synchronize()
            assert (J.value > 1) if pipeline else (J.value == 1)
            for r in range(P):
                for i in range(k):
                    what = f'{WIRE_NAME[wire]} P={P} round {t} rank {r} segment {i}'
                    assert_same(DT_FLOAT, to_host(outs[r][i], DT_FLOAT), want_out[i], what + f' op {OPS[i]}')
                    if res[r][i] is not None:
                        assert_same(DT_FLOAT, to_host(res[r][i], DT_FLOAT), want_res[r][i], what + ' residual')


def test_thread_world_feedback_is_race_free(lib, gpu):
    """The happens-before check over a pipelined feedback plan: the residuals are listed as
    accesses of the pack ('pack cvt fb'), and no pair of ops on them is unordered."""
    P, k = 3, len(ELEMENTS)
    ins = [[torch.ones(n, device=gpu) for n in ELEMENTS] for _ in range(P)]
    res = [[torch.zeros(n, device=gpu) for n in ELEMENTS] for _ in range(P)]
    S = (ctypes.c_void_p * (P * k))(*[x.data_ptr() for row in ins for x in row])
    R = (ctypes.c_void_p * (P * k))(*[x.data_ptr() for row in res for x in row])
    counts, report = (ctypes.c_longlong * 5)(), ctypes.create_string_buffer(1 << 14)
    with config(lib, reference_order=1, tune=0, fusion_pipeline_bytes=64 << 10):
        assert lib.ddl_testing_dep_trace(1) == 0
        try:
            for _ in range(2):
                st = lib.ddl_testing_thread_fused_allreduce_wire_fb(P, k, S, S, R, (ctypes.c_size_t * k)(*ELEMENTS),
                                                                    (ctypes.c_int * k)(*OPS), DT_BFLOAT16, _stream(), None)
                assert st == 0, lib.ddl_last_error()
        finally:
            torch.cuda.synchronize()
            assert lib.ddl_testing_dep_trace(0) == 0
    assert lib.ddl_testing_dep_check(counts, report, len(report)) == 0, lib.ddl_last_error()
    assert counts[0] > 0 and counts[4] == 0, report.value.decode()  # (ops, conflicts, ordered, ordered_reduce, races)


@pytest.fixture(scope='module')
def world(gpu):
    from ddl.torch.communicator import Communicator
    return Communicator.world()


def _rounds(world, name, n, comp, rounds, value=VALUE):
    """`rounds` requests of a constant tensor under one key: the value every round returned (all
    elements must agree)."""
    from ddl.torch.tensor_communicate import allreduce_async
    seen = []
    for _ in range(rounds):
        x = torch.full((n,), value, dtype=torch.float32, device='cuda')
        got = allreduce_async(x, name, world, compression=comp).wait(60).cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (n,) and (got == got[0]).all(), name
        seen.append(float(got[0]))
    return seen


N = 1029  # two tiles and a partial vector


@pytest.fixture
def data_plane(lib):
    with config(lib, one_rank_shortcut=0):
        yield


def test_handler_store_pinned_sequences(world, lib, gpu, data_plane):
    """One key, a constant gradient: the issue's pinned sequences with feedback; without it the
    small part is lost at every step."""
    from ddl.torch import Compression
    assert _rounds(world, 'fb_pin_bf16', N, Compression.bf16_feedback, 8) == BF16_SEQ
    assert _rounds(world, 'fb_pin_plain', N, Compression.bf16, 8) == [1.0] * 8
    assert _rounds(world, 'fb_pin_fp16', N, Compression.fp16_feedback, 8, 1 + 2.0 ** -13) == \
        [1, 1, 1, 1, 1.0009765625, 1, 1, 1]
    assert BF16_SEQ == constant_sequence(DT_BFLOAT16, VALUE, 8)[0]
    # an fp16 gradient of 1e-8 is zero for ever without feedback; with it, it reaches the wire
    assert _rounds(world, 'fb_tiny_plain', N, Compression.fp16, 4, 1e-8) == [0.0] * 4
    assert _rounds(world, 'fb_tiny', N, Compression.fp16_feedback, 8, 1e-8) == constant_sequence(DT_HALF, 1e-8, 8)[0]


def test_handler_store_restart_rules(world, lib, gpu, data_plane):
    from ddl.torch import Compression, config as cfg
    from ddl.torch.compression import reset_error_feedback
    fb = Compression.bf16_feedback
    old = cfg.get('wire_feedback_epoch')
    try:
        # reset_error_feedback() after round 3 restarts the sequence
        assert _rounds(world, 'fb_reset', N, fb, 3) == BF16_SEQ[:3]
        reset_error_feedback()
        assert _rounds(world, 'fb_reset', N, fb, 6) == BF16_SEQ[:6]
    finally:
        cfg.set('wire_feedback_epoch', old)
    # another element count restarts it (and so does the first count coming back)
    assert _rounds(world, 'fb_count', N, fb, 3) == BF16_SEQ[:3]
    assert _rounds(world, 'fb_count', 2 * N + 3, fb, 5) == BF16_SEQ[:5]
    assert _rounds(world, 'fb_count', N, fb, 5) == BF16_SEQ[:5]
    # a round without the bit in between leaves the residual where it was
    assert _rounds(world, 'fb_between', N, fb, 2) == BF16_SEQ[:2]
    assert _rounds(world, 'fb_between', N, Compression.bf16, 1) == [1.0]
    assert _rounds(world, 'fb_between', N, Compression.none, 1) == [VALUE]
    assert _rounds(world, 'fb_between', N, fb, 4) == BF16_SEQ[2:6]


def test_handler_store_in_a_batch(world, lib, gpu, data_plane):
    """Feedback, plain-wire and uncompressed requests in one batch under stable keys: the feedback
    keys follow the pinned sequence, the others do not move."""
    from ddl.torch import Compression, cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async_batch
    names = ['fb_batch_a', 'fb_batch_b', 'fb_batch_half']
    for t in range(6):
        ts = [torch.full((n,), VALUE, device='cuda') for n in (N, 70_001)] + [torch.ones(333, device='cuda').half()]
        hs = allreduce_async_batch(ts, names, world, op=cb.OP_AVG, compression=Compression.bf16_feedback)
        got = [h.wait(60) for h in hs]
        for g in got[:2]:
            assert g.dtype == torch.float32 and (g == BF16_SEQ[t]).all(), f'round {t}'
        assert got[2].dtype == torch.float16 and (got[2] == 1).all()


def test_one_rank_shortcut_touches_nothing(world, lib, gpu):
    """one_rank_shortcut 1: the input comes back bit for bit, also when the bit reaches the engine
    (the Python API does not even set it), and no residual is made: the data plane then starts the
    key from zero."""
    from ddl.torch import Compression, cpp_backend as cb
    done = cb.DONE_FN(lambda status, user: None)
    with config(lib, one_rank_shortcut=1):
        assert _rounds(world, 'fb_shortcut', N, Compression.bf16_feedback, 2) == [VALUE] * 2
        for _ in range(4):
            x = torch.full((N,), VALUE, dtype=torch.float32, device='cuda')
            st = lib.ddl_allreduce_submit_mem(world.id, b'fb_shortcut', x.data_ptr(), x.data_ptr(), N, DT_FLOAT,
                                              OP_SUM | WIRE_BF16 | WIRE_FEEDBACK, cb.MEMORY_DEVICE, _stream(), done, None)
            assert st == 0, lib.ddl_last_error()
            assert lib.ddl_wait_all(world.id) == 0
            torch.cuda.synchronize()
            assert (x == VALUE).all()
    with config(lib, one_rank_shortcut=0):
        assert _rounds(world, 'fb_shortcut', N, Compression.bf16_feedback, 5) == BF16_SEQ[:5]


def test_refusals(world, lib, gpu):
    """Every refusal of the contract, before anything is registered; after each group the
    communicator still runs a feedback request."""
    from ddl.torch import Compression, cpp_backend as cb
    done = cb.DONE_FN(lambda status, user: None)
    n = 16
    f32, f32h = torch.ones(n, device='cuda'), torch.ones(n)
    keys, users, n1 = (ctypes.c_char_p * 1)(b'fb_refused'), (ctypes.c_void_p * 1)(None), (ctypes.c_size_t * 1)(n)
    works = iter(range(100))

    def still_works():
        assert lib.ddl_wait_all(world.id) == 0  # nothing was registered
        with config(lib, one_rank_shortcut=0):
            assert _rounds(world, f'fb_after_refusal_{next(works)}', N, Compression.bf16_feedback, 5) == BF16_SEQ[:5]

    def submit(t, dt, op, mem):
        p = t.data_ptr()
        one, dts = (ctypes.c_void_p * 1)(p), (ctypes.c_int * 1)(dt)
        got = [lib.ddl_allreduce_submit_mem(world.id, b'fb_refused', p, p, n, dt, op, mem, _stream(), done, None),
               lib.ddl_allreduce_submit_batch_mem(world.id, 1, keys, one, one, n1, dts, op, mem, _stream(), done, users)]
        if mem == cb.MEMORY_DEVICE:
            got += [lib.ddl_allreduce_submit(world.id, b'fb_refused', p, p, n, dt, op, _stream(), done, None),
                    lib.ddl_allreduce_submit_batch(world.id, 1, keys, one, one, n1, dts, op, _stream(), done, users)]
        assert len(set(got)) == 1, (hex(op), got)
        return got[0]

    FB = WIRE_FEEDBACK
    # the bit without a wire flag, and with both
    for op in (FB, FB | OP_AVG, FB | WIRE_FP16 | WIRE_BF16, FB | WIRE_FP16 | WIRE_BF16 | OP_AVG):
        assert submit(f32, DT_FLOAT, op, cb.MEMORY_DEVICE) == INVALID_ARGUMENT, hex(op)
    assert submit(torch.ones(n, device='cuda').half(), DT_HALF, FB, cb.MEMORY_DEVICE) == INVALID_ARGUMENT
    still_works()
    # the unkeyed entry points
    p, one = f32.data_ptr(), (ctypes.c_void_p * 1)(f32.data_ptr())
    for op in (FB, FB | WIRE_FP16, FB | WIRE_BF16 | OP_AVG):
        assert lib.ddl_allreduce(world.id, p, p, n, DT_FLOAT, op, _stream()) == INVALID_ARGUMENT
        assert lib.ddl_allreduce_batch(world.id, 1, one, one, n1, DT_FLOAT, op, _stream()) == INVALID_ARGUMENT
        assert lib.ddl_allreduce_host(world.id, f32h.data_ptr(), f32h.data_ptr(), n, DT_FLOAT, op) == INVALID_ARGUMENT
    still_works()
    # host memory and other dtypes: the wire's own refusals, unchanged
    for flag in (WIRE_FP16, WIRE_BF16):
        for op in (FB | flag, FB | flag | OP_AVG):
            assert submit(f32h, DT_FLOAT, op, cb.MEMORY_HOST) == INVALID_ARGUMENT
            for dt, tdt in ((DT_HALF, torch.float16), (DT_BFLOAT16, torch.bfloat16), (DT_DOUBLE, torch.float64),
                            (DT_INT32, torch.int32)):
                assert submit(torch.ones(n, dtype=tdt, device='cuda'), dt, op, cb.MEMORY_DEVICE) == UNSUPPORTED_DTYPE
    still_works()
    # the other unknown bits stay refused, with and without the new one
    for op in (0x400, 0x80, 2, -1, 0x400 | FB | WIRE_FP16, 0x80 | FB | WIRE_BF16, 2 | FB | WIRE_BF16, 0x2000 | WIRE_FP16,
               0x800 | FB | WIRE_FP16):
        assert submit(f32, DT_FLOAT, op, cb.MEMORY_DEVICE) == INVALID_ARGUMENT, hex(op)
    still_works()
    assert torch.equal(f32, torch.ones(n, device='cuda'))
