"""The native bfloat16 statistic and factors through the engine on one GPU: the keyed path's FusionPipe on
every virtual rank (thread world, ddl_testing_thread_fused_allreduce_native) unpipelined and cut into sub-plans,
with the happens-before check; then the keyed handler at size 1 with the data plane on (one_rank_shortcut 0):
a request cut by 64 KiB plans, single-request plans with out != in, the shortcut itself, and the refusals.

Expected: the model of _bf16_native_helpers.py over the oracle's bf16 sum in the plan's MPICH order."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _bf16_native_helpers as bh
from _avg_helpers import to_dev, to_host
from _bf16_native_helpers import OP_AVG, OP_SUM, THIRD, THREE, assert_same, same_double
from _helpers import config
from _scale_helpers import LENS, SCALE

pytestmark = pytest.mark.gpu
DT_FLOAT, DT_DOUBLE, DT_INT32, DT_BFLOAT16, DT_HALF = 1, 2, 3, 14, 19
OP_MIN, OP_MAX = 3, 4
INVALID_ARGUMENT, UNSUPPORTED_DTYPE = 3, 4
ELEMS = [n for n in LENS if n]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _floats(values):
    return (ctypes.c_float * len(values))(*[float(v) for v in values])


def _thread_run(lib, gpu, P, xs, ops, pre=None, post=None, want=None, in_place=False):
    """One fused bf16 allreduce of the thread world over xs[r][i] (uint16). pre / post / want all None: the
    plain _ops entry. Returns (outputs [r][i], sub-plans, sums of squares or None, cuts)."""
    k = len(xs[0])
    ins = [[to_dev(x, gpu) for x in row] for row in xs]
    outs = ins if in_place else [[torch.zeros_like(t) for t in row] for row in ins]
    S = (ctypes.c_void_p * (P * k))(*[t.data_ptr() for row in ins for t in row])
    D = (ctypes.c_void_p * (P * k))(*[t.data_ptr() for row in outs for t in row])
    c_ops = (ctypes.c_int * k)(*ops)
    J, ncuts = ctypes.c_size_t(), ctypes.c_int()
    sq, cs, ce = None, (ctypes.c_size_t * 64)(), (ctypes.c_size_t * 64)()
    if pre is None and post is None and want is None:
        st = lib.ddl_testing_thread_fused_allreduce_ops(P, k, S, D, (ctypes.c_size_t * k)(*[2 * len(x) for x in xs[0]]),
                                                        c_ops, DT_BFLOAT16, _stream(), ctypes.byref(J))
    else:
        if want is not None:
            sq = (ctypes.c_double * (P * k))(*([-1.0] * (P * k)))
        st = lib.ddl_testing_thread_fused_allreduce_native(
            P, k, S, D, (ctypes.c_size_t * k)(*[len(x) for x in xs[0]]), c_ops, DT_BFLOAT16,
            _floats(pre) if pre is not None else None, _floats(post) if post is not None else None, _stream(),
            ctypes.byref(J), (ctypes.c_ubyte * k)(*want) if want is not None else None, sq, cs, ce, 64, ctypes.byref(ncuts))
    assert st == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    cuts = {}
    for c in range(ncuts.value):
        cuts.setdefault(cs[c], []).append(ce[c])
    return [[to_host(t, DT_BFLOAT16) for t in row] for row in outs], J.value, (list(sq) if sq is not None else None), cuts


@pytest.fixture(scope='module')
def thread_results():
    """(P, pipeline) -> (outputs, sums of squares, cuts) of test_thread_world_fused, for the comparison of the
    pipelined run with the unpipelined one."""
    return {}


@pytest.mark.parametrize('pipeline', [0, 64 << 10], ids=['unpipelined', 'subplans'])
@pytest.mark.parametrize('P', [2, 3])
def test_thread_world_fused(lib, gpu, oracle, thread_results, P, pipeline):
    k = len(ELEMS)
    ops = [OP_AVG if i % 2 else OP_SUM for i in range(k)]
    pre, post = bh.mixed_factors(k, 0), bh.mixed_factors(k, 1)  # post: 1/3 on AVG segments at P = 3, 3 among them
    want = [1 if i % 4 < 3 else 0 for i in range(k)]
    plan_bytes = sum(2 * n for n in ELEMS)
    xs = [[bh.native_input(n, 1000 * P + 10 * r + i) for i, n in enumerate(ELEMS)] for r in range(P)]
    with config(lib, reference_order=1, tune=0, fusion_pipeline_bytes=pipeline):
        got, J, sq, cuts = _thread_run(lib, gpu, P, xs, ops, pre, post, want)
    assert (J > 1) == bool(pipeline)
    assert bool(cuts) == bool(pipeline)
    for i in range(k):
        model = bh.expected(oracle, [xs[r][i] for r in range(P)], plan_bytes, ops[i], pre[i], post[i])
        for r in range(P):
            assert_same(got[r][i], model, f'rank {r} segment {i} (pre {pre[i]}, post {post[i]}, op {ops[i]})')
            assert got[r][i].tobytes() == got[0][i].tobytes()
            v = sq[r * k + i]
            m = bh.sumsq(got[r][i], cuts.get(i, ())) if want[i] else 0.0
            assert same_double(v, m), (r, i, v, m)
            assert same_double(v, sq[i])
    # finite data: the doubles are compared as bits; every segment wanted, in place
    ys = [[bh.native_input(n, 77 * P + 10 * r + i, specials=False) for i, n in enumerate(ELEMS)] for r in range(P)]
    with config(lib, reference_order=1, tune=0, fusion_pipeline_bytes=pipeline):
        fin, _, fsq, fcuts = _thread_run(lib, gpu, P, ys, ops, pre, post, [1] * k, in_place=True)
    for i in range(k):
        model = bh.expected(oracle, [ys[r][i] for r in range(P)], plan_bytes, ops[i], pre[i], post[i])
        for r in range(P):
            assert fin[r][i].tobytes() == model.tobytes(), (r, i)
            m = bh.sumsq(model, fcuts.get(i, ()))
            assert math.isfinite(m) and same_double(fsq[r * k + i], m), (r, i)
    thread_results[(P, pipeline)] = (got, fin)
    other = thread_results.get((P, (64 << 10) - pipeline))
    if other:  # the results are the same with and without the cuts (the statistic's pieces differ by design)
        for a, b in zip(other, (got, fin)):
            assert all(x.tobytes() == y.tobytes() for ra, rb in zip(a, b) for x, y in zip(ra, rb))


def test_plain_requests_unchanged_and_mixed_launches(lib, gpu):
    """Factors of 1 and nothing wanted through the native entry: the plain entry's bytes; one option on one
    segment leaves the other segments' bytes as they were."""
    xs = [[bh.native_input(n, 5 + 10 * r + i) for i, n in enumerate(ELEMS)] for r in range(2)]
    k = len(ELEMS)
    ops = [i % 2 for i in range(k)]
    ones = [1.0] * k
    with config(lib, reference_order=1, tune=0, fusion_pipeline_bytes=64 << 10):
        ref, _, _, _ = _thread_run(lib, gpu, 2, xs, ops)
        got, _, _, _ = _thread_run(lib, gpu, 2, xs, ops, ones, ones)
        post = list(ones)
        post[2] = THIRD
        mixed, _, sq, _ = _thread_run(lib, gpu, 2, xs, ops, ones, post, [1] + [0] * (k - 1))
    for r in range(2):
        for i, (g, m, w) in enumerate(zip(got[r], mixed[r], ref[r])):
            assert g.tobytes() == w.tobytes()
            if i != 2:
                assert m.tobytes() == w.tobytes()
        assert same_double(sq[r * k], bh.sumsq(ref[r][0]))


def test_thread_world_is_race_free(lib, gpu):
    """The happens-before check over a pipelined bf16 plan with factors and the statistic, in place."""
    P, k = 3, len(ELEMS)
    xs = [[np.full(n, 0x3f80, np.uint16) for n in ELEMS] for _ in range(P)]
    counts, report = (ctypes.c_longlong * 5)(), ctypes.create_string_buffer(1 << 14)
    with config(lib, reference_order=1, tune=0, fusion_pipeline_bytes=64 << 10):
        assert lib.ddl_testing_dep_trace(1) == 0
        try:
            got, J, _, _ = _thread_run(lib, gpu, P, xs, [OP_AVG] * k, [0.5] * k, [THIRD] * k, [1] * k, in_place=True)
            assert J > 1
        finally:
            torch.cuda.synchronize()
            assert lib.ddl_testing_dep_trace(0) == 0
    assert lib.ddl_testing_dep_check(counts, report, len(report)) == 0, lib.ddl_last_error()
    assert counts[0] > 0 and counts[4] == 0, report.value.decode()  # (ops, conflicts, ordered, ordered_reduce, races)
    # 1 (x) 0.5 on every rank, the sum 1.5 = 0x3fc0, (/) 3, (x) 1/3, one rounding
    assert all((g == bh.unpack(np.array([0x3fc0], np.uint16), OP_AVG, 3, THIRD)[0]).all() for row in got for g in row)


@pytest.fixture(scope='module')
def world(gpu):
    from ddl.torch.communicator import Communicator
    return Communicator.world()


def _dev(x):
    return torch.from_numpy(x.view(np.int16)).cuda().view(torch.bfloat16)


def _host(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.mark.parametrize('shortcut', [0, 1])
def test_size_one_world(world, lib, shortcut):
    """Keyed bf16 requests at P = 1: stored = narrow(widen(narrow(widen(g) (x) a)) (x) b), each step skipped when
    its factor is 1; with the shortcut (g (x) a) (x) b by two in-place launches, the same bits."""
    from ddl.torch import cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async, allreduce_async_batch
    tag = f'bn1_{shortcut}'

    def model(x, a, b):
        return bh.unpack(bh.pack(x, a), OP_SUM, 1, b)
    with config(lib, one_rank_shortcut=shortcut, fusion_pipeline_bytes=0):
        x = bh.native_input(70_001, 1)
        # a single-request plan with out != in: postscale and the statistic, then prescale, then both, in place
        src = _dev(x)
        h = allreduce_async(src, f'{tag}_post', world, op=cb.OP_AVG, postscale=float(THIRD), sumsq=True)
        out = _host(h.wait(60))
        assert_same(out, model(x, 1.0, THIRD))
        assert _host(src).tobytes() == x.tobytes()
        assert same_double(h.sumsq, bh.sumsq(out))
        h = allreduce_async(_dev(x), f'{tag}_pre', world, prescale=float(THIRD))
        assert_same(_host(h.wait(60)), model(x, THIRD, 1.0))
        t = _dev(x)[1:]  # 2-byte aligned only
        h = allreduce_async(t, f'{tag}_both', world, output=t, prescale=float(THIRD), postscale=3.0, sumsq=True)
        assert h.wait(60) is t
        assert_same(_host(t), model(x[1:], THIRD, THREE))
        assert same_double(h.sumsq, bh.sumsq(_host(t)))
        y = bh.native_input(4099, 9, specials=False)
        h = allreduce_async(_dev(y), f'{tag}_stat', world, sumsq=True)  # the statistic alone: the bytes, read in place
        out = _host(h.wait(60))
        assert out.tobytes() == y.tobytes() and math.isfinite(h.sumsq) and same_double(h.sumsq, bh.sumsq(y))
        # a fused plan mixing requests with and without the options
        lens = [5, 300, 4099, 70_001, 1, 0, 513]
        pre, post = bh.mixed_factors(len(lens), 1), bh.mixed_factors(len(lens), 3)
        xs = [bh.native_input(n, 40 + i) for i, n in enumerate(lens)]
        ts = [_dev(v) for v in xs]
        wishes = [i % 2 == 0 for i in range(len(ts))]
        hs = allreduce_async_batch(ts, [f'{tag}_b{i}' for i in range(len(ts))], world, outputs=ts, op=cb.OP_AVG,
                                   prescale=[float(a) for a in pre], postscale=[float(b) for b in post], sumsq=wishes)
        for i, (v, t, hh) in enumerate(zip(xs, ts, hs)):
            hh.wait(60)
            assert_same(_host(t), model(v, pre[i], post[i]), f'batch {i}')
            if pre[i] == 1 and post[i] == 1:
                assert _host(t).tobytes() == v.tobytes()
            assert (hh.sumsq is not None) == wishes[i]
            if wishes[i]:
                assert same_double(hh.sumsq, bh.sumsq(_host(t))), i
        # 64 KiB plans: the 70 001-element request spans plans, its statistic cut where the plans end
        with config(lib, fusion_threshold_bytes=64 << 10):
            ys = [bh.native_input(n, 70 + i, specials=False) for i, n in enumerate((5, 300, 70_001))]
            hs = allreduce_async_batch([_dev(v) for v in ys], [f'{tag}_p{i}' for i in range(3)], world,
                                       prescale=[1.0, float(THIRD), float(THIRD)], postscale=[3.0, 1.0, 3.0], sumsq=True)
            outs = [_host(hh.wait(60)) for hh in hs]
        before = 2 * (5 + 300)
        cuts = [(j * (64 << 10) - before) // 2 for j in range(1, 4) if (j * (64 << 10) - before) // 2 < 70_001]
        assert len(cuts) == 2
        for i, (v, o, hh, a, b, c) in enumerate(zip(ys, outs, hs, (1.0, THIRD, THIRD), (THREE, 1.0, THREE), ((), (), cuts))):
            assert o.tobytes() == model(v, a, b).tobytes(), i
            assert math.isfinite(hh.sumsq) and same_double(hh.sumsq, bh.sumsq(o, c)), (i, hh.sumsq)
        # plain bf16 requests: the bytes they had
        u = bh.native_input(70_001, 4)
        h0 = allreduce_async(_dev(u), f'{tag}_plain', world, op=cb.OP_AVG)
        h1 = allreduce_async(_dev(u), f'{tag}_ones', world, op=cb.OP_AVG, prescale=1.0, postscale=1.0)
        assert _host(h0.wait(60)).tobytes() == _host(h1.wait(60)).tobytes() == u.tobytes()


def test_refusals(world, lib):
    """What stays refused, before anything is registered; the communicator works afterwards."""
    from ddl.torch import cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async
    done = cb.DONE_FN(lambda status, user: None)
    bf = torch.ones(16, dtype=torch.bfloat16, device='cuda')
    tensors = {DT_HALF: torch.ones(16, dtype=torch.float16, device='cuda'),
               DT_DOUBLE: torch.ones(16, dtype=torch.float64, device='cuda'),
               DT_INT32: torch.ones(16, dtype=torch.int32, device='cuda')}
    hbf = torch.ones(16, dtype=torch.bfloat16)
    count = [0]

    def works():
        count[0] += 1
        x = _dev(bh.native_input(1000, count[0], specials=False))
        h = allreduce_async(x, f'bn_after_refusal_{count[0]}', world, postscale=0.5, sumsq=True)
        assert_same(_host(h.wait(60)), bh.unpack(_host(x), OP_SUM, 1, 0.5))

    def submit(t, dt, op, mem, arg):
        return lib.ddl_allreduce_submit_mem(world.id, b'bn_refused', t.data_ptr(), t.data_ptr(), 16, dt, op, mem, _stream(),
                                            done, ctypes.addressof(arg))

    def submit_batch(t, dt, op, mem, arg):
        one = (ctypes.c_void_p * 1)(t.data_ptr())
        return lib.ddl_allreduce_submit_batch_mem(world.id, 1, (ctypes.c_char_p * 1)(b'bn_refused'), one, one,
                                                  (ctypes.c_size_t * 1)(16), (ctypes.c_int * 1)(dt), op, mem, _stream(), done,
                                                  (ctypes.c_void_p * 1)(ctypes.addressof(arg)))
    v = (ctypes.c_double * 1)(-1.0)
    scale = cb.ScaleArg(None, None, 0.5, 2.0)
    stat = cb.SumsqArg(None, ctypes.addressof(v))
    for fn in (submit, submit_batch):
        for bit, arg in ((SCALE, scale), (cb.SUMSQ, stat)):
            for dt, t in tensors.items():
                assert fn(t, dt, OP_SUM | bit, cb.MEMORY_DEVICE, arg) == UNSUPPORTED_DTYPE, (dt, bit)
                assert lib.ddl_last_error()
            assert fn(hbf, DT_BFLOAT16, OP_SUM | bit, cb.MEMORY_HOST, arg) == INVALID_ARGUMENT
            assert fn(bf, DT_BFLOAT16, OP_MIN | bit, cb.MEMORY_DEVICE, arg) == INVALID_ARGUMENT
            assert fn(bf, DT_BFLOAT16, OP_MAX | bit, cb.MEMORY_DEVICE, arg) == INVALID_ARGUMENT
        for bad in (0.0, -1.0, math.inf, math.nan):
            for arg in (cb.ScaleArg(None, None, bad, 1.0), cb.ScaleArg(None, None, 1.0, bad)):
                assert fn(bf, DT_BFLOAT16, OP_SUM | SCALE, cb.MEMORY_DEVICE, arg) == INVALID_ARGUMENT, bad
        works()
    assert lib.ddl_wait_all(world.id) == 0
    torch.cuda.synchronize()
    assert v[0] == -1.0 and (bf == 1).all() and (hbf == 1).all()  # nothing ran
    # accepted: SCALE | SUMSQ on bf16, the double from the same struct
    t = torch.full((16,), 3.0, dtype=torch.bfloat16, device='cuda')
    arg = cb.ScaleArg(None, ctypes.addressof(v), 0.5, 1.0)
    assert submit(t, DT_BFLOAT16, OP_SUM | SCALE | cb.SUMSQ, cb.MEMORY_DEVICE, arg) == 0 and lib.ddl_wait_all(world.id) == 0
    torch.cuda.synchronize()
    assert v[0] == 16 * 1.5 * 1.5 and (t == 1.5).all()
