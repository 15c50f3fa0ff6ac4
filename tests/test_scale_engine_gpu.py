"""The scale factors through the engine on one GPU: the keyed path's FusionPipe on every virtual rank
(thread world) with per-request factors, unpipelined and cut into sub-plans, uncompressed and over both
wires; the motivating fp16 overflow; the size-1 world's keyed requests (direct plans, fused plans,
requests spanning plans, the one-rank shortcut); unscaled requests unchanged; the refusals.

Expected: the UNSCALED engine entries run on NumPy-prescaled inputs with SUM give the reduced stream;
NumPy takes the quotient and the postscale (_scale_helpers.result). A NaN must be a NaN."""
import ctypes
import math
import struct

import numpy as np
import pytest
import torch

from _helpers import config
from _scale_helpers import LENS, OP_AVG, OP_SUM, SCALE, mixed_factors, mul, result, same_bits, scale_input
from _sumsq_helpers import mirror
from _wire_helpers import narrow, widen

pytestmark = pytest.mark.gpu
DT_FLOAT, DT_INT32, DT_BFLOAT16, DT_HALF = 1, 3, 14, 19
OP_MIN, OP_MAX = 3, 4
INVALID_ARGUMENT, UNSUPPORTED_DTYPE = 3, 4
ELEMS = [n for n in LENS if n]  # the thread world's entries take non-empty segments as the sumsq test does
HALF = np.float32(0.5)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(v):
    return struct.pack('<d', v)


def _floats(values):
    return (ctypes.c_float * len(values))(*[float(v) for v in values])


def _thread_run(lib, gpu, P, xs, ops, wire, pre=None, post=None, want=None):
    """One fused allreduce of the thread world over xs[r][i]; pre / post None: the unscaled entries.
    Returns (outputs [r][i] as numpy, sub-plans, sums of squares or None, cuts)."""
    k = len(xs[0])
    ins = [[torch.from_numpy(x).to(gpu) for x in row] for row in xs]
    outs = [[torch.zeros_like(t) for t in row] for row in ins]
    S = (ctypes.c_void_p * (P * k))(*[t.data_ptr() for row in ins for t in row])
    D = (ctypes.c_void_p * (P * k))(*[t.data_ptr() for row in outs for t in row])
    n_arr = (ctypes.c_size_t * k)(*[len(x) for x in xs[0]])
    c_ops = (ctypes.c_int * k)(*ops)
    J, ncuts = ctypes.c_size_t(), ctypes.c_int()
    sq, cs, ce = None, (ctypes.c_size_t * 64)(), (ctypes.c_size_t * 64)()
    if pre is None and post is None:
        if wire:
            st = lib.ddl_testing_thread_fused_allreduce_wire(P, k, S, D, n_arr, c_ops, wire, _stream(), ctypes.byref(J))
        else:
            st = lib.ddl_testing_thread_fused_allreduce_ops(P, k, S, D, (ctypes.c_size_t * k)(*[4 * len(x) for x in xs[0]]),
                                                            c_ops, DT_FLOAT, _stream(), ctypes.byref(J))
    else:
        if want is not None:
            sq = (ctypes.c_double * (P * k))(*([-1.0] * (P * k)))
        st = lib.ddl_testing_thread_fused_allreduce_scale(
            P, k, S, D, None, n_arr, c_ops, wire, _floats(pre) if pre is not None else None,
            _floats(post) if post is not None else None, _stream(), ctypes.byref(J),
            (ctypes.c_ubyte * k)(*want) if want is not None else None, sq, cs, ce, 64, ctypes.byref(ncuts))
    assert st == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    cuts = {}
    for c in range(ncuts.value):
        cuts.setdefault(cs[c], []).append(ce[c])
    return [[t.cpu().numpy() for t in row] for row in outs], J.value, (list(sq) if sq is not None else None), cuts


@pytest.mark.parametrize('pipeline', [0, 256 << 10], ids=['unpipelined', 'subplans'])
@pytest.mark.parametrize('wire', [0, DT_HALF, DT_BFLOAT16], ids=['fp32', 'fp16', 'bf16'])
@pytest.mark.parametrize('P', [2, 3])
def test_thread_world_fused(lib, gpu, P, wire, pipeline):
    k = len(ELEMS)
    ops = [i % 2 for i in range(k)]
    pre, post = mixed_factors(k, 0), mixed_factors(k, 2)
    want = [1 if i % 4 < 2 else 0 for i in range(k)]
    xs = [[scale_input(n, 1000 * P + 10 * r + i, pre[i]) for i, n in enumerate(ELEMS)] for r in range(P)]
    with config(lib, reference_order=1, tune=0, fusion_pipeline_bytes=pipeline):
        sums, J0, _, _ = _thread_run(lib, gpu, P, [[mul(x, pre[i]) for i, x in enumerate(row)] for row in xs],
                                     [OP_SUM] * k, wire)
        got, J, sq, cuts = _thread_run(lib, gpu, P, xs, ops, wire, pre, post, want)
    assert J == J0 and (J > 1) == bool(pipeline)
    for r in range(P):
        for i in range(k):
            model = result(sums[r][i], ops[i], P, post[i])
            assert same_bits(got[r][i], model), f'rank {r} segment {i} (pre {pre[i]}, post {post[i]}, op {ops[i]})'
            assert same_bits(got[r][i], got[0][i])
            v = sq[r * k + i]
            if want[i]:
                m = mirror(got[r][i], bool(wire), cuts.get(i, ()))
                assert (math.isnan(v) and math.isnan(m)) or _bits(v) == _bits(m), (r, i, v, m)
                assert (math.isnan(v) and math.isnan(sq[i])) or _bits(v) == _bits(sq[i])
            else:
                assert _bits(v) == _bits(0.0)
    # finite data: the doubles are compared as bits
    rng = np.random.default_rng(P)
    xs = [[rng.standard_normal(n).astype(np.float32) for n in ELEMS] for _ in range(P)]
    with config(lib, reference_order=1, tune=0, fusion_pipeline_bytes=pipeline):
        got, _, sq, cuts = _thread_run(lib, gpu, P, xs, ops, wire, pre, post, [1] * k)
    for r in range(P):
        for i in range(k):
            m = mirror(got[r][i], bool(wire), cuts.get(i, ()))
            assert math.isfinite(m) and _bits(sq[r * k + i]) == _bits(m), (r, i)


def test_fp16_overflow_in_the_sum(lib, gpu):
    """Both ranks hold 40000: the fp16 sum is inf; with prescale 0.5 it is exactly 40000."""
    xs = [[np.full(1000, 40000.0, np.float32)] for _ in range(2)]
    with config(lib, reference_order=1, tune=0, fusion_pipeline_bytes=0):
        plain, _, _, _ = _thread_run(lib, gpu, 2, xs, [OP_SUM], DT_HALF)
        assert np.isinf(plain[0][0]).all()
        a, _, _, _ = _thread_run(lib, gpu, 2, xs, [OP_SUM], DT_HALF, [HALF], [1.0])
        b, _, _, _ = _thread_run(lib, gpu, 2, xs, [OP_AVG], DT_HALF, [HALF], [2.0])
    for r in range(2):
        assert (a[r][0] == 40000.0).all() and (b[r][0] == 40000.0).all()


def test_unscaled_requests_unchanged(lib, gpu):
    """Factors of 1 through the scaled entry: the parent entries' bytes."""
    rng = np.random.default_rng(3)
    xs = [[rng.standard_normal(n).astype(np.float32) for n in ELEMS] for _ in range(2)]
    ops = [i % 2 for i in range(len(ELEMS))]
    ones = [1.0] * len(ELEMS)
    for wire in (0, DT_BFLOAT16):
        with config(lib, reference_order=1, tune=0, fusion_pipeline_bytes=256 << 10):
            ref, _, _, _ = _thread_run(lib, gpu, 2, xs, ops, wire)
            got, _, _, _ = _thread_run(lib, gpu, 2, xs, ops, wire, ones, ones)
        for r in range(2):
            for g, w in zip(got[r], ref[r]):
                assert g.tobytes() == w.tobytes()


@pytest.fixture(scope='module')
def world(gpu):
    from ddl.torch.communicator import Communicator
    return Communicator.world()


@pytest.mark.parametrize('shortcut', [1, 0])
def test_size_one_world(world, lib, shortcut):
    """Keyed requests at P = 1: out = (g (x) a) (x) b, each factor skipped when it is 1."""
    from ddl.torch import cpp_backend as cb
    from ddl.torch.compression import Compression
    from ddl.torch.tensor_communicate import allreduce_async, allreduce_async_batch
    tag = f'sc1_{shortcut}'
    third, f3 = np.float32(1.0 / 3.0), np.float32(3.0)

    def dev(x):
        return torch.from_numpy(x).cuda()
    with config(lib, one_rank_shortcut=shortcut, fusion_pipeline_bytes=0):
        x = scale_input(70_001, 1, third)
        # direct single-request plan, postscale only: in != out, then in place, AVG and SUM
        h = allreduce_async(dev(x), f'{tag}_post', world, postscale=float(third), sumsq=True)
        out = h.wait(60).cpu().numpy()
        assert same_bits(out, mul(x, third))
        m = mirror(out, False)
        assert (math.isnan(m) and math.isnan(h.sumsq)) or _bits(m) == _bits(h.sumsq)
        t = dev(x)
        h = allreduce_async(t, f'{tag}_post_inplace', world, output=t, op=cb.OP_AVG, postscale=3.0)
        assert h.wait(60) is t and same_bits(t.cpu().numpy(), mul(x, f3))
        # direct single-request plan with a prescale (one in-place launch ahead of the in-place allreduce off the shortcut), and with both
        h = allreduce_async(dev(x), f'{tag}_pre', world, prescale=float(third))
        assert same_bits(h.wait(60).cpu().numpy(), mul(x, third))
        t = dev(x)[1:]  # 4-byte aligned only
        h = allreduce_async(t, f'{tag}_both', world, output=t, prescale=float(third), postscale=3.0, sumsq=True)
        h.wait(60)
        assert same_bits(t.cpu().numpy(), mul(mul(x[1:], third), f3))
        y = np.random.default_rng(9).standard_normal(4099).astype(np.float32)
        h = allreduce_async(dev(y), f'{tag}_finite', world, op=cb.OP_AVG, prescale=0.5, postscale=float(third), sumsq=True)
        out = h.wait(60).cpu().numpy()
        assert out.tobytes() == mul(mul(y, 0.5), third).tobytes() and _bits(h.sumsq) == _bits(mirror(out, False))
        # a fused plan: scaled and unscaled requests, SUM / AVG alike at P = 1
        lens = [5, 300, 4099, 70_001, 1, 0, 513]
        pre, post = mixed_factors(len(lens), 1), mixed_factors(len(lens), 4)
        xs = [scale_input(n, 40 + i, pre[i]) for i, n in enumerate(lens)]
        ts = [dev(v) for v in xs]
        hs = allreduce_async_batch(ts, [f'{tag}_b{i}' for i in range(len(ts))], world, outputs=ts, op=cb.OP_AVG,
                                   prescale=[float(a) for a in pre], postscale=[float(b) for b in post],
                                   sumsq=[i % 2 == 0 for i in range(len(ts))])
        for i, (v, t, hh) in enumerate(zip(xs, ts, hs)):
            hh.wait(60)
            assert same_bits(t.cpu().numpy(), mul(mul(v, pre[i]), post[i])), i
            if pre[i] == 1 and post[i] == 1:
                assert t.cpu().numpy().tobytes() == v.tobytes()
            if i % 2 == 0:
                m = mirror(t.cpu().numpy(), False)
                assert (math.isnan(m) and math.isnan(hh.sumsq)) or _bits(m) == _bits(hh.sumsq), i
        # 64 KiB plans: the last request spans plans
        with config(lib, fusion_threshold_bytes=64 << 10):
            ys = [scale_input(n, 70 + i, third) for i, n in enumerate((5, 300, 70_001))]
            hs = allreduce_async_batch([dev(v) for v in ys], [f'{tag}_p{i}' for i in range(3)], world,
                                       prescale=[1.0, float(third), float(third)], postscale=[3.0, 1.0, 3.0])
            outs = [hh.wait(60).cpu().numpy() for hh in hs]
        assert same_bits(outs[0], mul(ys[0], f3)) and same_bits(outs[1], mul(ys[1], third))
        assert same_bits(outs[2], mul(mul(ys[2], third), f3))
        if not shortcut:  # the data plane runs, and the wire with it: narrow(g (x) a), widened, (x) b
            z = np.random.default_rng(2).standard_normal(4099).astype(np.float32)
            h = allreduce_async(dev(z), f'{tag}_wire', world, compression=Compression.bf16, prescale=float(third),
                                postscale=3.0)
            want = mul(widen(DT_BFLOAT16, narrow(DT_BFLOAT16, mul(z, third))), f3)
            assert h.wait(60).cpu().numpy().tobytes() == want.tobytes()
        # unscaled requests: the parent's bytes
        u = np.random.default_rng(4).standard_normal(70_001).astype(np.float32)
        h0 = allreduce_async(dev(u), f'{tag}_plain', world, op=cb.OP_AVG)
        h1 = allreduce_async(dev(u), f'{tag}_ones', world, op=cb.OP_AVG, prescale=1.0, postscale=1.0)
        assert h0.wait(60).cpu().numpy().tobytes() == h1.wait(60).cpu().numpy().tobytes() == u.tobytes()


def test_refusals(world, lib):
    """Every refusal of the contract, each followed by a successful plain request on the communicator."""
    from ddl.torch import cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async
    done = cb.DONE_FN(lambda status, user: None)
    f32 = torch.ones(16, device='cuda')
    i32 = torch.ones(16, dtype=torch.int32, device='cuda')
    f16 = torch.ones(16, dtype=torch.float16, device='cuda')
    h32 = torch.ones(16)
    count = [0]

    def works():
        count[0] += 1
        x = torch.randn(1000, device='cuda')
        assert torch.equal(allreduce_async(x, f'sc_after_refusal_{count[0]}', world).wait(60), x)

    def submit(t, dt, op, mem, arg):
        user = ctypes.addressof(arg) if arg is not None else None
        return lib.ddl_allreduce_submit_mem(world.id, b'sc_refused', t.data_ptr(), t.data_ptr(), 16, dt, op, mem, _stream(),
                                            done, user)

    def submit_batch(t, dt, op, mem, arg):
        users = (ctypes.c_void_p * 1)(ctypes.addressof(arg)) if arg is not None else None
        one = (ctypes.c_void_p * 1)(t.data_ptr())
        return lib.ddl_allreduce_submit_batch_mem(world.id, 1, (ctypes.c_char_p * 1)(b'sc_refused'), one, one,
                                                  (ctypes.c_size_t * 1)(16), (ctypes.c_int * 1)(dt), op, mem, _stream(), done,
                                                  users)
    for bad in (0.0, -1.0, math.inf, math.nan):
        for arg in (cb.ScaleArg(None, None, bad, 1.0), cb.ScaleArg(None, None, 1.0, bad)):
            for fn in (submit, submit_batch):
                assert fn(f32, DT_FLOAT, OP_SUM | SCALE, cb.MEMORY_DEVICE, arg) == INVALID_ARGUMENT, bad
                assert lib.ddl_last_error()
        works()
    half = cb.ScaleArg(None, None, 0.5, 1.0)
    post = cb.ScaleArg(None, None, 1.0, 2.0)
    for arg in (half, post):
        for fn in (submit, submit_batch):
            assert fn(i32, DT_INT32, OP_SUM | SCALE, cb.MEMORY_DEVICE, arg) == UNSUPPORTED_DTYPE
            assert fn(f16, DT_HALF, OP_AVG | SCALE, cb.MEMORY_DEVICE, arg) == UNSUPPORTED_DTYPE
            works()
            assert fn(h32, DT_FLOAT, OP_SUM | SCALE, cb.MEMORY_HOST, arg) == INVALID_ARGUMENT
            works()
            assert fn(f32, DT_FLOAT, OP_MIN | SCALE, cb.MEMORY_DEVICE, arg) == INVALID_ARGUMENT
            assert fn(f32, DT_FLOAT, OP_MAX | SCALE, cb.MEMORY_DEVICE, arg) == INVALID_ARGUMENT
            works()
    for fn in (submit, submit_batch):  # a NULL user
        assert fn(f32, DT_FLOAT, OP_SUM | SCALE, cb.MEMORY_DEVICE, None) == INVALID_ARGUMENT
    works()
    # the bit on the unkeyed entries
    assert lib.ddl_allreduce(world.id, f32.data_ptr(), f32.data_ptr(), 16, DT_FLOAT, OP_SUM | SCALE, _stream()) == INVALID_ARGUMENT
    one = (ctypes.c_void_p * 1)(f32.data_ptr())
    assert lib.ddl_allreduce_batch(world.id, 1, one, one, (ctypes.c_size_t * 1)(16), DT_FLOAT, OP_SUM | SCALE,
                                   _stream()) == INVALID_ARGUMENT
    assert lib.ddl_allreduce_host(world.id, h32.data_ptr(), h32.data_ptr(), 16, DT_FLOAT, OP_SUM | SCALE) == INVALID_ARGUMENT
    assert lib.ddl_wait_all(world.id) == 0
    assert torch.equal(f32.cpu(), torch.ones(16)) and torch.equal(h32, torch.ones(16))  # nothing ran
    works()
    # both factors 1: the request without the bit, also for what the factors refuse
    ones = cb.ScaleArg(None, None, 1.0, 1.0)
    assert submit(i32, DT_INT32, OP_MAX | SCALE, cb.MEMORY_DEVICE, ones) == 0
    assert lib.ddl_wait_all(world.id) == 0
    # SCALE | SUMSQ: sumsq from the same struct; without the SUMSQ bit it is ignored
    v = (ctypes.c_double * 1)(-1.0)
    t = torch.full((16,), 3.0, device='cuda')
    arg = cb.ScaleArg(None, ctypes.addressof(v), 0.5, 1.0)
    assert submit(t, DT_FLOAT, OP_SUM | SCALE, cb.MEMORY_DEVICE, arg) == 0 and lib.ddl_wait_all(world.id) == 0
    torch.cuda.synchronize()
    assert v[0] == -1.0 and (t == 1.5).all()
    assert submit(t, DT_FLOAT, OP_SUM | SCALE | cb.SUMSQ, cb.MEMORY_DEVICE, arg) == 0 and lib.ddl_wait_all(world.id) == 0
    torch.cuda.synchronize()
    assert v[0] == 16 * 0.75 * 0.75 and (t == 0.75).all()
