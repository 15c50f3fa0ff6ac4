"""Error feedback of the e4m3 wire through the engine on one GPU: the thread world at P = 2, 3, 8 and 16 with
caller-owned residuals over two steps (factors, the statistic, pipeline cuts inside requests, segments with and
without residuals in one plan); the keyed handler at size 1 with the data plane on (plan cuts, every restart rule,
the one-rank shortcut); the refusals; the data-parallel wrapper in two processes. Everything is compared bit for bit
with the CPU model of _e4m3_feedback_helpers.py."""
import ctypes
import math
import struct

import numpy as np
import pytest
import torch

import _e4m3_feedback_helpers as fb
import _e4m3_helpers as q8
from _avg_helpers import assert_same
from _helpers import config
from _sumsq_helpers import mirror

pytestmark = pytest.mark.gpu
DT_FLOAT, DT_INT32, DT_HALF = 1, 3, 19
OP_SUM, OP_AVG, OP_MIN, OP_MAX = 0, 1, 3, 4
INVALID_ARGUMENT, UNSUPPORTED_DTYPE = 3, 4
F = np.float32
THIRD = float(F(1) / F(3))
LENS = q8.ENGINE_LENS
Q, QF = q8.WIRE_E4M3, fb.WIRE_E4M3_FEEDBACK
OPS = [i % 2 for i in range(len(LENS))]
PRE = [1.0, THIRD, 1.0, 0.5]
POST = [1.0, 1.0, THIRD, THIRD]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(v):
    return struct.pack('<d', v)


def _floats(values):
    return (ctypes.c_float * len(values))(*[float(v) for v in values])


def _thread_step(lib, gpu, P, xs, res, status=0):
    """One fused e4m3 allreduce of the thread world over xs[r][i] with the residual tensors res[r][i] (None: that
    rank's segment has none), OPS / PRE / POST and every statistic. Returns (outputs [r][i], sub-plans, sums of
    squares, cuts by segment)."""
    k = len(xs[0])
    ins = [[torch.from_numpy(x).to(gpu) for x in row] for row in xs]
    outs = [[torch.full_like(t, 7.0) for t in row] for row in ins]
    VP = ctypes.c_void_p * (P * k)
    S, D = VP(*[t.data_ptr() for row in ins for t in row]), VP(*[t.data_ptr() for row in outs for t in row])
    R = VP(*[t.data_ptr() if t is not None else None for row in res for t in row])
    J, ncuts = ctypes.c_size_t(), ctypes.c_int()
    cs, ce = (ctypes.c_size_t * 64)(), (ctypes.c_size_t * 64)()
    sq = (ctypes.c_double * (P * k))(*([-1.0] * (P * k)))
    st = lib.ddl_testing_thread_fused_allreduce_e4m3_fb(
        P, k, S, D, R, (ctypes.c_size_t * k)(*[len(x) for x in xs[0]]), (ctypes.c_int * k)(*OPS[:k]), _floats(PRE[:k]),
        _floats(POST[:k]), _stream(), ctypes.byref(J), (ctypes.c_ubyte * k)(*([1] * k)), sq, cs, ce, 64, ctypes.byref(ncuts))
    assert st == status, lib.ddl_last_error()
    torch.cuda.synchronize()
    cuts = {}
    for c in range(ncuts.value):
        cuts.setdefault(cs[c], []).append(ce[c])
    for row_in, row in zip(ins, xs):
        for t, x in zip(row_in, row):
            assert t.cpu().numpy().tobytes() == x.tobytes(), 'an input was written'
    return [[t.cpu().numpy() for t in row] for row in outs], J.value, list(sq), cuts


@pytest.fixture(scope='module')
def models():
    """The model's two steps of the shared inputs, computed once per (P, which segments carry a residual)."""
    cache = {}

    def get(P, mixed):
        if (P, mixed) not in cache:
            steps = [fb.step_inputs(P, LENS, q8.ENGINE_SEED, t) for t in range(2)]
            has = [[not mixed or (r + i) % 2 == 0 for i in range(len(LENS))] for r in range(P)]
            want = [fb.allreduce_steps([[steps[t][r][i] for r in range(P)] for t in range(2)], OPS[i], PRE[i], POST[i],
                                       feedback=[has[r][i] for r in range(P)]) for i in range(len(LENS))]
            cache[P, mixed] = (steps, has, want)
        return cache[P, mixed]
    return get


@pytest.mark.parametrize('how', ['unpipelined', 'pipelined', 'mixed'])
@pytest.mark.parametrize('P', q8.ENGINE_RANKS)
def test_thread_world_is_the_model(lib, gpu, models, P, how):
    """Two consecutive steps on the residuals the first one left: SUM and AVG requests with factors and the
    statistic. `pipelined`: fusion_pipeline_bytes 4096, so pieces start inside requests and a piece's residual must
    start at the piece's first element. `mixed`: the same with every other (rank, request) without a residual."""
    k = len(LENS)
    steps, has, want = models(P, how == 'mixed')
    res = [[torch.zeros(n, device=gpu) if has[r][i] else None for i, n in enumerate(LENS)] for r in range(P)]
    with config(lib, tune=0, fusion_pipeline_bytes=0 if how == 'unpipelined' else 4096):
        for t in range(2):
            got, J, sq, cuts = _thread_step(lib, gpu, P, steps[t], res)
            assert (J == 1) == (how == 'unpipelined')
            for r in range(P):
                for i in range(k):
                    what = f'{how} P={P} step {t} rank {r} request {i} ({J} sub-plans)'
                    assert_same(DT_FLOAT, got[r][i], want[i][0][t], what)
                    assert got[r][i].tobytes() == got[0][i].tobytes(), f'rank {r} differs from rank 0'
                    m, v = mirror(got[r][i], False, cuts.get(i, ())), sq[r * k + i]
                    assert (math.isnan(v) and math.isnan(m)) or _bits(v) == _bits(m), (what, v, m)
            if how != 'unpipelined':
                assert cuts.get(k - 1) and all(c % q8.G == 0 for v in cuts.values() for c in v)
    for r in range(P):
        for i in range(k):
            if has[r][i]:
                assert res[r][i].cpu().numpy().tobytes() == want[i][1][r].tobytes(), f'{how} P={P} residual {r} / {i}'


def test_seventeen_ranks_are_refused(lib, gpu):
    xs = [[np.ones(300, F)] for _ in range(17)]
    res = [[torch.zeros(300, device=gpu)] for _ in range(17)]
    _thread_step(lib, gpu, 17, xs, res, status=INVALID_ARGUMENT)
    assert b'16' in lib.ddl_last_error()
    assert all(not t[0].any() for t in res)


# ---- the keyed handler at size 1 with the data plane on -------------------------------------------------------------
@pytest.fixture(scope='module')
def world(gpu):
    from ddl.torch.communicator import Communicator
    return Communicator.world()


N = 70_001


def _x(t, n=N, specials=False):
    return q8.rank_input(n, 900 + t, specials=specials)


def _send(world, name, x, compression, **kw):
    from ddl.torch.tensor_communicate import allreduce_async
    src = torch.from_numpy(x).cuda()
    out = allreduce_async(src, name, world, compression=compression, **kw).wait(60)
    assert src.cpu().numpy().tobytes() == x.tobytes()
    return out.cpu().numpy()


def _model(x, r, op=OP_SUM, pre=1.0, post=1.0):
    w, r = fb.pack_fb(x, np.zeros(x.size, F) if r is None else r, pre)
    return q8.unpack(w, x.size, op, 1, post), r


def test_handler_three_steps_cut_by_plans(world, lib):
    """A request of 70 001 elements cut by 64 KiB plans (256 granules each), three steps under one name, AVG with a
    prescale, a postscale and the statistic; the first step holds NaNs and infinities."""
    from ddl.torch import Compression, cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async
    r = None
    with config(lib, one_rank_shortcut=0, fusion_pipeline_bytes=0, fusion_threshold_bytes=64 << 10):
        for t in range(3):
            x = _x(t, specials=t == 0)
            h = allreduce_async(torch.from_numpy(x).cuda(), 'q8fb_cut', world, compression=Compression.fp8_feedback,
                                op=cb.OP_AVG, prescale=THIRD, postscale=3.0, sumsq=True)
            out = h.wait(60).cpu().numpy()
            want, r = _model(x, r, OP_AVG, THIRD, 3.0)
            assert_same(DT_FLOAT, out, want, f'step {t}')
            assert math.isnan(h.sumsq) == (t == 0)
    with config(lib, one_rank_shortcut=0, fusion_pipeline_bytes=4096):  # the fourth step through sub-plans
        x = _x(3)
        want, r = _model(x, r, OP_SUM, THIRD)
        assert_same(DT_FLOAT, _send(world, 'q8fb_cut', x, Compression.fp8_feedback, prescale=THIRD), want, 'sub-plans')


def test_handler_restart_rules(world, lib):
    from ddl.torch import Compression, config as cfg
    from ddl.torch.compression import reset_error_feedback
    k = Compression.fp8_feedback
    x0, x1, x2 = _x(10, 5003), _x(11, 5003), _x(12, 5003)
    w0, r0 = _model(x0, None)
    fresh1, carried1 = _model(x1, None)[0], _model(x1, r0)[0]
    assert fresh1.tobytes() != carried1.tobytes()  # the inputs tell a restart from a carry-over
    with config(lib, one_rank_shortcut=0):
        old = cfg.get('wire_feedback_epoch')
        try:  # reset_error_feedback() between two steps restarts it
            assert _send(world, 'q8fb_reset', x0, k).tobytes() == w0.tobytes()
            reset_error_feedback()
            assert _send(world, 'q8fb_reset', x1, k).tobytes() == fresh1.tobytes()
        finally:
            cfg.set('wire_feedback_epoch', old)
        # another element count restarts it, and so does the first count coming back
        assert _send(world, 'q8fb_count', x0, k).tobytes() == w0.tobytes()
        y = _x(13, 2 * 5003 + 3)
        assert _send(world, 'q8fb_count', y, k).tobytes() == _model(y, None)[0].tobytes()
        assert _send(world, 'q8fb_count', x1, k).tobytes() == fresh1.tobytes()
        # the same name under bf16_feedback, then fp8_feedback: from zero; and back again: bf16 from zero
        bf = lambda v: torch.from_numpy(v).to(torch.bfloat16).float().numpy()  # noqa: E731
        assert _send(world, 'q8fb_family', x0, Compression.bf16_feedback).tobytes() == bf(x0).tobytes()
        assert _send(world, 'q8fb_family', x1, k).tobytes() == fresh1.tobytes()
        assert _send(world, 'q8fb_family', x2, Compression.bf16_feedback).tobytes() == bf(x2).tobytes()
        # (fp16 <-> bf16 keeps the residual: tests/test_feedback_engine_gpu.py)
        # a step without the bit neither reads nor changes it
        assert _send(world, 'q8fb_between', x0, k).tobytes() == w0.tobytes()
        assert _send(world, 'q8fb_between', x2, Compression.fp8).tobytes() == q8.allreduce([x2]).tobytes()
        assert _send(world, 'q8fb_between', x2, Compression.none).tobytes() == x2.tobytes()
        assert _send(world, 'q8fb_between', x1, k).tobytes() == carried1.tobytes()


def test_one_rank_shortcut_touches_nothing(world, lib):
    from ddl.torch import Compression, cpp_backend as cb
    done = cb.DONE_FN(lambda status, user: None)
    x0, x1 = _x(20, 5003), _x(21, 5003)
    with config(lib, one_rank_shortcut=1):
        assert _send(world, 'q8fb_shortcut', x0, Compression.fp8_feedback).tobytes() == x0.tobytes()
        t = torch.from_numpy(x0).cuda()  # also when the bits reach the engine (the Python API does not set them)
        st = lib.ddl_allreduce_submit_mem(world.id, b'q8fb_shortcut', t.data_ptr(), t.data_ptr(), x0.size, DT_FLOAT,
                                          OP_SUM | Q | QF, cb.MEMORY_DEVICE, _stream(), done, None)
        assert st == 0, lib.ddl_last_error()
        assert lib.ddl_wait_all(world.id) == 0
        torch.cuda.synchronize()
        assert t.cpu().numpy().tobytes() == x0.tobytes()
    with config(lib, one_rank_shortcut=0):  # no residual was made: the data plane starts the key from zero
        assert _send(world, 'q8fb_shortcut', x1, Compression.fp8_feedback).tobytes() == _model(x1, None)[0].tobytes()


def test_refusals(world, lib):
    """Every row of the contract's refusal table, before anything is registered; a plain request works afterwards."""
    from ddl.torch import Compression, cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async
    done = cb.DONE_FN(lambda status, user: None)
    n = 16
    f32, h32 = torch.ones(n, device='cuda'), torch.ones(n)
    keys, users, n1 = (ctypes.c_char_p * 1)(b'q8fb_refused'), (ctypes.c_void_p * 1)(None), (ctypes.c_size_t * 1)(n)

    def submit(t, dt, op, mem):
        p = t.data_ptr()
        one, dts = (ctypes.c_void_p * 1)(p), (ctypes.c_int * 1)(dt)
        got = [lib.ddl_allreduce_submit_mem(world.id, b'q8fb_refused', p, p, n, dt, op, mem, _stream(), done, None),
               lib.ddl_allreduce_submit_batch_mem(world.id, 1, keys, one, one, n1, dts, op, mem, _stream(), done, users)]
        if mem == cb.MEMORY_DEVICE:
            got += [lib.ddl_allreduce_submit(world.id, b'q8fb_refused', p, p, n, dt, op, _stream(), done, None),
                    lib.ddl_allreduce_submit_batch(world.id, 1, keys, one, one, n1, dts, op, _stream(), done, users)]
        assert len(set(got)) == 1, (hex(op), got)
        assert lib.ddl_last_error()
        return got[0]

    dev = cb.MEMORY_DEVICE
    for base in (OP_SUM, OP_AVG):
        assert submit(f32, DT_FLOAT, base | QF, dev) == INVALID_ARGUMENT  # the bit without WIRE_E4M3
        for wire in (cb.WIRE_FP16, cb.WIRE_BF16):
            assert submit(f32, DT_FLOAT, base | QF | wire, dev) == INVALID_ARGUMENT
            assert submit(f32, DT_FLOAT, base | Q | QF | wire, dev) == INVALID_ARGUMENT
            assert submit(f32, DT_FLOAT, base | QF | wire | cb.WIRE_FEEDBACK, dev) == INVALID_ARGUMENT
        for other in (cb.WIRE_FEEDBACK, cb.WIRE_STOCHASTIC, cb.WIRE_BF16 | cb.WIRE_STOCHASTIC):
            assert submit(f32, DT_FLOAT, base | Q | QF | other, dev) == INVALID_ARGUMENT, hex(other)
        assert submit(f32, DT_FLOAT, base | Q | cb.WIRE_FEEDBACK, dev) == INVALID_ARGUMENT  # stays refused
        assert submit(h32, DT_FLOAT, base | Q | QF, cb.MEMORY_HOST) == INVALID_ARGUMENT
        assert submit(torch.ones(n, dtype=torch.int32, device='cuda'), DT_INT32, base | Q | QF, dev) == UNSUPPORTED_DTYPE
        assert submit(torch.ones(n, dtype=torch.float16, device='cuda'), DT_HALF, base | Q | QF, dev) == UNSUPPORTED_DTYPE
    for op in (OP_MIN, OP_MAX):
        assert submit(f32, DT_FLOAT, op | Q | QF, dev) == INVALID_ARGUMENT
        assert submit(f32, DT_FLOAT, op | QF, dev) == INVALID_ARGUMENT
    # the unkeyed entry points
    p, one = f32.data_ptr(), (ctypes.c_void_p * 1)(f32.data_ptr())
    for op in (Q | QF, QF, OP_AVG | Q | QF):
        assert lib.ddl_allreduce(world.id, p, p, n, DT_FLOAT, op, _stream()) == INVALID_ARGUMENT
        assert lib.ddl_allreduce_batch(world.id, 1, one, one, n1, DT_FLOAT, op, _stream()) == INVALID_ARGUMENT
        assert lib.ddl_allreduce_host(world.id, h32.data_ptr(), h32.data_ptr(), n, DT_FLOAT, op) == INVALID_ARGUMENT
    # the old unknown bits stay refused, with and without the new bit
    for bit in (0x80, 0x400, 0x800, 0x10000, 2, 5, -1):
        for with_new in (0, Q | QF, QF):
            assert submit(f32, DT_FLOAT, bit | with_new, dev) == INVALID_ARGUMENT, (hex(bit), hex(with_new))
    with pytest.raises(ValueError):
        allreduce_async(f32, 'q8fb_minmax', world, op=cb.OP_MAX, compression=Compression.fp8_feedback)
    assert lib.ddl_wait_all(world.id) == 0
    assert torch.equal(f32.cpu(), torch.ones(n)) and torch.equal(h32, torch.ones(n))  # nothing ran
    x = torch.randn(1000, device='cuda')
    assert torch.equal(allreduce_async(x, 'q8fb_after_refusals', world).wait(60), x)
    with config(lib, one_rank_shortcut=0):  # and the bit itself, with the statistic and the factors OR-ed in
        v = _x(30, 1009)
        h = allreduce_async(torch.from_numpy(v).cuda(), 'q8fb_after_refusals', world, compression=Compression.fp8_feedback,
                            op=cb.OP_AVG, prescale=0.5, postscale=2.0, sumsq=True)
        want = _model(v, None, OP_AVG, 0.5, 2.0)[0]
        assert h.wait(60).cpu().numpy().tobytes() == want.tobytes() and _bits(h.sumsq) == _bits(mirror(want, False))


def test_dp_wrapper_in_two_processes(gpu):
    """Two optimizer steps of a three-parameter model with compression=Compression.fp8_feedback equal the model (a
    world of one rank does not communicate in the wrapper, so this is two processes over the test transport:
    tests/_mp_e4m3_feedback_worker.check_e4m3_fb_wrapper)."""
    from test_e4m3_feedback_multiproc_gpu import _run
    _run(2, ['check_e4m3_fb_wrapper'], 'gloo')
