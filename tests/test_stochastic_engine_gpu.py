"""Stochastic rounding of the bf16 wire through the engine on one GPU: the compressed fusion plan of every
virtual rank with caller-supplied stream keys (thread world, unpipelined and cut into sub-plans, with the sum
of squares and a postscale on top), the keyed handler's own stream keys through the Python API on a one-rank
world, the contrast with the plain bf16 wire the feature exists for, and the refusals.

Expected values: _stochastic_helpers (the header's R, rule and host mix in NumPy) for every rank's wire
values, then the oracle's sum of the wire values in MPICH's order for the plan's unpadded wire bytes, widened,
divided by np.float32(P) where the op is AVG — bit for bit."""
import ctypes
import math
import struct

import numpy as np
import pytest
import torch

import _stochastic_helpers as sh
from _avg_helpers import assert_same, to_dev, to_host
from _feedback_helpers import WIRE_FEEDBACK, reduce_ref
from _helpers import DT_BFLOAT16, DT_DOUBLE, DT_FLOAT, DT_HALF, DT_INT32, config
from _scale_helpers import result, same_bits
from _sumsq_helpers import mirror
from _wire_helpers import OP_AVG, OP_SUM, WIRE_BF16, WIRE_FP16, widen, wire_input

pytestmark = pytest.mark.gpu
INVALID_ARGUMENT, UNSUPPORTED_DTYPE = 3, 4
SR = sh.WIRE_STOCHASTIC
ELEMENTS = [5, 300, 70_001, 4099, 1, 513]  # 70_001 elements = 140 KB on the wire: cut by a 64 KiB pipeline
OPS = [i % 2 for i in range(len(ELEMENTS))]  # SUM, AVG, SUM, ...
PLAIN = {3}  # the segment without the bit: one launch mixes both
POST = [1.0, 0.5, 1.0 / 3.0, 1.0, 3.0, 2.0 ** -16]
N = 1029  # two tiles and a partial vector


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _key(P, r, i):
    return sh.mix64((P << 20) | (r << 10) | i)


@pytest.fixture(scope='module')
def model(oracle):
    """P -> (inputs [r][i], every rank's wire values, the reduced widened stream per segment): computed once
    per P on first use, shared by all runs, never written to."""
    cache = {}

    def get(P):
        if P not in cache:
            k, message = len(ELEMENTS), 2 * sum(ELEMENTS)
            xs = [[wire_input(n, 5300 + 101 * P + 17 * r + i) for i, n in enumerate(ELEMENTS)] for r in range(P)]
            ws = [[sh.sr_or_cast(xs[r][i], None if i in PLAIN else _key(P, r, i)) for i in range(k)] for r in range(P)]
            sums = [reduce_ref(oracle, DT_BFLOAT16, [ws[r][i] for r in range(P)], message, OP_SUM, P) for i in range(k)]
            for a in [x for row in xs for x in row] + sums:
                a.setflags(write=False)
            cache[P] = (xs, ws, sums)
        return cache[P]
    return get


def _run(lib, gpu, P, xs, post=None, want=None):
    k = len(ELEMENTS)
    ins = [[to_dev(x.copy(), gpu) for x in row] for row in xs]
    outs = [[torch.zeros_like(x) for x in row] for row in ins]
    S = (ctypes.c_void_p * (P * k))(*[x.data_ptr() for row in ins for x in row])
    D = (ctypes.c_void_p * (P * k))(*[x.data_ptr() for row in outs for x in row])
    J, ncuts = ctypes.c_size_t(), ctypes.c_int()
    cs, ce = (ctypes.c_size_t * 64)(), (ctypes.c_size_t * 64)()
    sq = (ctypes.c_double * (P * k))(*([-1.0] * (P * k))) if want is not None else None
    st = lib.ddl_testing_thread_fused_allreduce_wire_sr(
        P, k, S, D, (ctypes.c_size_t * k)(*ELEMENTS), (ctypes.c_int * k)(*OPS),
        (ctypes.c_ubyte * k)(*[int(i not in PLAIN) for i in range(k)]),
        (ctypes.c_ulonglong * (P * k))(*[_key(P, r, i) for r in range(P) for i in range(k)]), None,
        (ctypes.c_float * k)(*post) if post is not None else None, _stream(), ctypes.byref(J),
        (ctypes.c_ubyte * k)(*want) if want is not None else None, sq, cs, ce, 64, ctypes.byref(ncuts))
    assert st == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    cuts = {}
    for c in range(ncuts.value):
        cuts.setdefault(cs[c], []).append(ce[c])
    return [[to_host(t, DT_FLOAT) for t in row] for row in outs], J.value, (list(sq) if sq is not None else None), cuts


@pytest.mark.parametrize('P', [3, 8])
def test_thread_world_stochastic_plan(lib, gpu, model, P):
    """Every rank's output is the bf16 wire mirror applied to the mirror-rounded inputs, SUM and AVG; cut into
    sub-plans (the 70_001-element segment across three of them) no bit changes: an element's random bits are
    those of its index in the request."""
    xs, _, sums = model(P)
    runs = {}
    for pipeline in (0, 64 << 10):
        with config(lib, reference_order=1, tune=0, fusion_pipeline_bytes=pipeline):
            runs[pipeline], J, _, _ = _run(lib, gpu, P, xs)
        assert (J > 1) if pipeline else (J == 1)
        for r in range(P):
            for i in range(len(ELEMENTS)):
                assert_same(DT_FLOAT, runs[pipeline][r][i], result(sums[i], OPS[i], P, 1.0),
                            f'P={P} pipeline {pipeline} rank {r} segment {i} op {OPS[i]}')
    for r in range(P):
        for i in range(len(ELEMENTS)):
            assert same_bits(runs[0][r][i], runs[64 << 10][r][i])


@pytest.mark.parametrize('pipeline', [0, 64 << 10], ids=['unpipelined', 'pipelined'])
def test_thread_world_with_sumsq_and_postscale(lib, gpu, model, pipeline):
    P, k = 3, len(ELEMENTS)
    xs, _, sums = model(P)
    want = [1, 1, 1, 0, 1, 1]
    with config(lib, reference_order=1, tune=0, fusion_pipeline_bytes=pipeline):
        got, J, sq, cuts = _run(lib, gpu, P, xs, POST, want)
    assert (J > 1) == bool(pipeline) and bool(cuts) == bool(pipeline)
    for r in range(P):
        for i in range(k):
            assert same_bits(got[r][i], result(sums[i], OPS[i], P, POST[i])), f'rank {r} segment {i}'
            v, m = sq[r * k + i], mirror(got[r][i], True, cuts.get(i, ())) if want[i] else 0.0
            assert (math.isnan(v) and math.isnan(m)) or struct.pack('<d', v) == struct.pack('<d', m), (r, i, v, m)


@pytest.fixture(scope='module')
def world(gpu):
    from ddl.torch.communicator import Communicator
    return Communicator.world()


@pytest.fixture
def data_plane(lib):
    with config(lib, one_rank_shortcut=0):
        yield


@pytest.fixture
def seeded(lib):
    """Restores the process's seed."""
    old = lib.ddl_get_config(b'wire_stochastic_seed')
    yield
    assert lib.ddl_set_config(b'wire_stochastic_seed', old) == 0


def _call(world, name, x, comp, **kw):
    from ddl.torch.tensor_communicate import allreduce_async
    got = allreduce_async(torch.from_numpy(x).cuda(), name, world, compression=comp, **kw).wait(60).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == x.shape
    return got


def test_keyed_requests_follow_the_host_mix(world, lib, gpu, data_plane, seeded):
    """One stable name, three calls: call n is widen(SR(x; S(seed, 0, name, n))); the three differ; after
    set_stochastic_seed the next call follows the new seed (the key's sequence number runs on)."""
    from ddl.torch import Compression
    from ddl.torch.compression import set_stochastic_seed
    name, x = 'sr_keyed', wire_input(N, 5900)
    set_stochastic_seed(1234)
    assert lib.ddl_get_config(b'wire_stochastic_seed') == 1234
    got = [_call(world, name, x, Compression.bf16_stochastic) for _ in range(3)]
    for n, g in enumerate(got):
        assert_same(DT_FLOAT, g, widen(DT_BFLOAT16, sh.sr(x, sh.stream(1234, 0, name, n))), f'call {n}')
    assert not same_bits(got[0], got[1]) and not same_bits(got[1], got[2]) and not same_bits(got[0], got[2])
    set_stochastic_seed(2 ** 64 - 3)  # all 64 bits are the seed
    g = _call(world, name, x, Compression.bf16_stochastic)
    assert_same(DT_FLOAT, g, widen(DT_BFLOAT16, sh.sr(x, sh.stream(2 ** 64 - 3, 0, name, 3))), 'after the new seed')
    # a request of the key without the bit spends no sequence number, and AVG at P = 1 is SUM
    assert_same(DT_FLOAT, _call(world, name, x, Compression.bf16), widen(DT_BFLOAT16, sh.sr_or_cast(x, None)), 'plain')
    from ddl.torch import cpp_backend as cb
    g = _call(world, name, x, Compression.bf16_stochastic, op=cb.OP_AVG)
    assert_same(DT_FLOAT, g, widen(DT_BFLOAT16, sh.sr(x, sh.stream(2 ** 64 - 3, 0, name, 4))), 'sequence number 4')


def test_keyed_request_cut_by_plans_and_pipeline(world, lib, gpu, data_plane, seeded):
    """The wire values do not depend on fusion_threshold_bytes or fusion_pipeline_bytes: the same request
    (fresh names, so sequence number 0; the stream key follows the name) cut into plans and sub-plans."""
    from ddl.torch import Compression
    x = wire_input(70_001, 5901)
    for t, (thr, pipe) in enumerate([(64 << 20, 0), (48 << 10, 0), (64 << 20, 32 << 10), (40 << 10, 16 << 10)]):
        name = f'sr_cut_{t}'
        with config(lib, fusion_threshold_bytes=thr, fusion_pipeline_bytes=pipe):
            g = _call(world, name, x, Compression.bf16_stochastic, prescale=0.5)
        S = sh.stream(lib.ddl_get_config(b'wire_stochastic_seed'), 0, name, 0)
        with np.errstate(all='ignore'):
            want = widen(DT_BFLOAT16, sh.sr((x * np.float32(0.5)).astype(np.float32), S))
        assert_same(DT_FLOAT, g, want, f'threshold {thr} pipeline {pipe}')


def test_the_bias_is_gone(world, lib, gpu, data_plane, seeded):
    """4096 elements of 1 + 2**-10, 64 steps under one name: the plain bf16 wire returns exactly 1.0 every step;
    with stochastic rounding the mean over the steps and elements is within 5 standard errors of the value."""
    from ddl.torch import Compression
    n, steps = 4096, 64
    x = np.full(n, sh.VALUE, np.float32)
    total = 0.0
    for _ in range(steps):
        assert (_call(world, 'sr_bias_plain', x, Compression.bf16) == 1.0).all()
        g = _call(world, 'sr_bias', x, Compression.bf16_stochastic)
        assert set(np.unique(g).tolist()) == {1.0, 1.0078125}
        total += float(g.astype(np.float64).sum())
    err = total / (n * steps) - float(np.float32(sh.VALUE))
    se = sh.SIGMA / math.sqrt(n * steps)
    print(f'mean error {err:.3e} = {err / se:+.2f} standard errors; the plain wire is off by {-2.0 ** -10 / se:.0f}')
    assert abs(err) <= 5 * se


def test_one_rank_shortcut_touches_nothing(world, lib, gpu, seeded):
    """one_rank_shortcut 1: the input comes back bit for bit, also when the bit reaches the engine (the Python
    API does not even set it), and no sequence number is spent: the data plane then starts the key at 0."""
    from ddl.torch import Compression, cpp_backend as cb
    done = cb.DONE_FN(lambda status, user: None)
    x = wire_input(N, 5902)
    finite = np.isfinite(x)
    with config(lib, one_rank_shortcut=1):
        assert same_bits(_call(world, 'sr_shortcut', x, Compression.bf16_stochastic), x)
        for _ in range(3):
            t = torch.from_numpy(x).cuda()
            st = lib.ddl_allreduce_submit_mem(world.id, b'sr_shortcut', t.data_ptr(), t.data_ptr(), N, DT_FLOAT,
                                              OP_SUM | WIRE_BF16 | SR, cb.MEMORY_DEVICE, _stream(), done, None)
            assert st == 0, lib.ddl_last_error()
            assert lib.ddl_wait_all(world.id) == 0
            torch.cuda.synchronize()
            assert same_bits(t.cpu().numpy(), x)
    with config(lib, one_rank_shortcut=0):
        g = _call(world, 'sr_shortcut', x, Compression.bf16_stochastic)
    assert_same(DT_FLOAT, g, widen(DT_BFLOAT16, sh.sr(x, sh.stream(lib.ddl_get_config(b'wire_stochastic_seed'), 0,
                                                                   'sr_shortcut', 0))), 'sequence number 0')
    assert finite.any()


def test_refusals(world, lib, gpu):
    """Every refusal of the contract, from every entry point, before anything is registered; after each group
    the communicator still runs a plain request and a stochastic one."""
    from ddl.torch import Compression, cpp_backend as cb
    done = cb.DONE_FN(lambda status, user: None)
    n = 16
    f32, f32h = torch.ones(n, device='cuda'), torch.ones(n)
    keys, users, n1 = (ctypes.c_char_p * 1)(b'sr_refused'), (ctypes.c_void_p * 1)(None), (ctypes.c_size_t * 1)(n)
    works = iter(range(100))
    x = np.full(N, sh.VALUE, np.float32)

    def still_works():
        assert lib.ddl_wait_all(world.id) == 0  # nothing was registered
        with config(lib, one_rank_shortcut=0):
            t = next(works)
            assert (_call(world, f'sr_after_refusal_plain_{t}', x, Compression.none) == x).all()
            g = _call(world, f'sr_after_refusal_{t}', x, Compression.bf16_stochastic)
            seed = lib.ddl_get_config(b'wire_stochastic_seed')
            assert_same(DT_FLOAT, g, widen(DT_BFLOAT16, sh.sr(x, sh.stream(seed, 0, f'sr_after_refusal_{t}', 0))), 'after')

    def submit(t, dt, op, mem):
        p = t.data_ptr()
        one, dts = (ctypes.c_void_p * 1)(p), (ctypes.c_int * 1)(dt)
        got = [lib.ddl_allreduce_submit_mem(world.id, b'sr_refused', p, p, n, dt, op, mem, _stream(), done, None),
               lib.ddl_allreduce_submit_batch_mem(world.id, 1, keys, one, one, n1, dts, op, mem, _stream(), done, users)]
        if mem == cb.MEMORY_DEVICE:
            got += [lib.ddl_allreduce_submit(world.id, b'sr_refused', p, p, n, dt, op, _stream(), done, None),
                    lib.ddl_allreduce_submit_batch(world.id, 1, keys, one, one, n1, dts, op, _stream(), done, users)]
        assert len(set(got)) == 1, (hex(op), got)
        return got[0]

    # the bit without WIRE_BF16, with WIRE_FP16 (alone or with BF16), with WIRE_FEEDBACK
    for op in (SR, SR | OP_AVG, SR | WIRE_FP16, SR | WIRE_FP16 | OP_AVG, SR | WIRE_FP16 | WIRE_BF16,
               SR | WIRE_BF16 | WIRE_FEEDBACK, SR | WIRE_BF16 | WIRE_FEEDBACK | OP_AVG, SR | WIRE_FP16 | WIRE_FEEDBACK,
               SR | WIRE_FEEDBACK):
        assert submit(f32, DT_FLOAT, op, cb.MEMORY_DEVICE) == INVALID_ARGUMENT, hex(op)
    assert submit(torch.ones(n, device='cuda').bfloat16(), DT_BFLOAT16, SR, cb.MEMORY_DEVICE) == INVALID_ARGUMENT
    still_works()
    # MIN / MAX
    for op in (SR | WIRE_BF16 | cb.OP_MIN, SR | WIRE_BF16 | cb.OP_MAX, SR | cb.OP_MIN, SR | cb.OP_MAX):
        assert submit(f32, DT_FLOAT, op, cb.MEMORY_DEVICE) == INVALID_ARGUMENT, hex(op)
    still_works()
    # the unkeyed entry points
    p, one = f32.data_ptr(), (ctypes.c_void_p * 1)(f32.data_ptr())
    for op in (SR, SR | WIRE_BF16, SR | WIRE_BF16 | OP_AVG):
        assert lib.ddl_allreduce(world.id, p, p, n, DT_FLOAT, op, _stream()) == INVALID_ARGUMENT
        assert lib.ddl_allreduce_batch(world.id, 1, one, one, n1, DT_FLOAT, op, _stream()) == INVALID_ARGUMENT
        assert lib.ddl_allreduce_host(world.id, f32h.data_ptr(), f32h.data_ptr(), n, DT_FLOAT, op) == INVALID_ARGUMENT
    still_works()
    # host memory, and other dtypes: the wire flag's own refusals
    for op in (SR | WIRE_BF16, SR | WIRE_BF16 | OP_AVG):
        assert submit(f32h, DT_FLOAT, op, cb.MEMORY_HOST) == INVALID_ARGUMENT
        for dt, tdt in ((DT_HALF, torch.float16), (DT_BFLOAT16, torch.bfloat16), (DT_DOUBLE, torch.float64),
                        (DT_INT32, torch.int32)):
            assert submit(torch.ones(n, dtype=tdt, device='cuda'), dt, op, cb.MEMORY_DEVICE) == UNSUPPORTED_DTYPE
    still_works()
    # the other unknown bits stay refused, with and without the new one
    for op in (0x400, 0x80, 0x800, 2, 5, 0x400 | SR | WIRE_BF16, 0x80 | SR | WIRE_BF16, 0x800 | SR | WIRE_BF16,
               2 | SR | WIRE_BF16, 5 | SR | WIRE_BF16, 0x10000 | SR | WIRE_BF16):
        assert submit(f32, DT_FLOAT, op, cb.MEMORY_DEVICE) == INVALID_ARGUMENT, hex(op)
    still_works()
    assert torch.equal(f32, torch.ones(n, device='cuda'))
    assert WIRE_FEEDBACK == 0x1000
