"""Every 16-bit pattern through the two-input reduce, the N-input folds and the converting pack
(csrc/reduce_kernels.hip, csrc/pack.hip k_seg<CvtPackOp>), in all their forms, plus an edge table for
fp32 / fp64 and one schedule-level check per 16-bit type.

The inputs are the sets of tests/_edge_helpers.py (every pattern against 26 partners: subnormals,
overflow to inf, NaNs with every payload, inf - inf, exact ties; tests/test_edge_values_cpu.py shows
on the CPU that they hold these and that a subtly wrong kernel would fail). Expected values are the
oracle's and the CPU's casts, never the engine's. Compared with assert_same: bit for bit where the
expected value is no NaN, a NaN where it is one. One launch per case of the 16-bit sets."""
import ctypes

import numpy as np
import pytest
import torch

import _edge_helpers as eh
from _avg_helpers import assert_same, to_host
from _avg_helpers import to_dev as _to_dev
from _helpers import NAME, NP, config, ring_perms, ring_shape
from _wire_helpers import WIRE_NAME, narrow

pytestmark = pytest.mark.gpu
VP, SZ = ctypes.c_void_p, ctypes.c_size_t
GUARD = 0xA5
BY_NAME = dict(ids=lambda d: NAME[d])
FOLD_NB = [1, 2, 7, 15]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def to_dev(x, gpu):
    return _to_dev(np.array(x), gpu)  # a copy: the cached sets are read-only, which torch.from_numpy warns about


def _ok(lib, st):
    assert st == 0, lib.ddl_last_error()
    torch.cuda.synchronize()


class _Shifted:
    """A host array on the device one element past a 16-byte boundary (the kernels' element paths), in
    an allocation filled with a guard byte."""

    def __init__(self, x, gpu, fill=True):
        self.n, self.es, self.dtype = x.size, x.itemsize, x.dtype
        host = np.full((x.size + 16) * x.itemsize, GUARD, np.uint8)
        if fill:
            host[self.es:self.es + x.nbytes] = np.ascontiguousarray(x).view(np.uint8)
        self.t = torch.from_numpy(host).to(gpu)
        self.ptr = self.t.data_ptr() + self.es
        assert self.t.data_ptr() % 16 == 0 and self.ptr % 16 != 0

    def result(self):
        """The n elements at the shifted pointer; nothing around them may have been written."""
        raw = self.t.cpu().numpy()
        lo, hi = self.es, self.es + self.n * self.es
        assert (raw[:lo] == GUARD).all() and (raw[hi:] == GUARD).all(), 'bytes outside the output were written'
        return raw[lo:hi].view(self.dtype)


# ---- the two-input reduce -------------------------------------------------------------------------
@pytest.fixture(scope='module')
def pair_case(oracle):
    """dt -> (a, b, the oracle's sum): the pair set and 7 more pairs (n mod 8 = 7: the tail lanes run)."""
    out = {}
    for dt in eh.HALF_TYPES:
        a, b = eh.pair_set(dt, tail=True)
        assert a.size % 8 == 7
        out[dt] = (a, b, oracle.sum2(dt, a, b))
    return out


SUM2_FORMS = ['sum2', 'local', 'lds_stage', 'run8', 'run4', 'offset']


@pytest.mark.parametrize('form', SUM2_FORMS)
@pytest.mark.parametrize('dt', eh.HALF_TYPES, **BY_NAME)
def test_sum2_every_pattern(lib, gpu, pair_case, dt, form):
    """ddl_reduce_sum2 out of place, ddl_reduce_local in place, the LDS-staged variant (8), the run
    forms (32|7: 8-tile runs, 96|7: 4-tile runs), and all three buffers one element off alignment (the
    scalar kernel: Add<>::one on every pattern)."""
    a, b, want = pair_case[dt]
    n = a.size
    if form == 'offset':
        sa, sb, so = _Shifted(a, gpu), _Shifted(b, gpu), _Shifted(a, gpu, fill=False)
        _ok(lib, lib.ddl_reduce_sum2(so.ptr, sa.ptr, sb.ptr, n, dt, _stream()))
        got = so.result()
    else:
        ta, tb = to_dev(a, gpu), to_dev(b, gpu)
        to = ta if form == 'local' else torch.zeros_like(ta)
        if form == 'sum2':
            st = lib.ddl_reduce_sum2(to.data_ptr(), ta.data_ptr(), tb.data_ptr(), n, dt, _stream())
        elif form == 'local':
            st = lib.ddl_reduce_local(ta.data_ptr(), tb.data_ptr(), n, dt, _stream())
        else:
            variant = {'lds_stage': 8, 'run8': 32 | 7, 'run4': 96 | 7}[form]
            st = lib.ddl_reduce_sum2_variant(variant, to.data_ptr(), ta.data_ptr(), tb.data_ptr(), n, dt, _stream())
        _ok(lib, st)
        got = to_host(to, dt)
        if form != 'local':
            assert to_host(ta, dt).tobytes() == a.tobytes() and to_host(tb, dt).tobytes() == b.tobytes()
    assert_same(dt, got.view(NP[dt]), want, f'{NAME[dt]} {form}')


# ---- the N-input folds ------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def fold_case(oracle):
    """(dt, nb) -> (x_0 .. x_nb, the oracle's fold), computed once."""
    cache = {}

    def get(dt, nb):
        if (dt, nb) not in cache:
            xs = eh.fold_set(dt, nb)
            cache[dt, nb] = (xs, oracle.fold(dt, xs))
        return cache[dt, nb]
    return get


FOLD_FORMS = ['fold', 'ordered1', 'ordered2', 'run_form', 'offset', 'batch']


@pytest.mark.parametrize('form', FOLD_FORMS)
@pytest.mark.parametrize('nb', FOLD_NB)
@pytest.mark.parametrize('dt', eh.HALF_TYPES, **BY_NAME)
def test_fold_every_pattern(lib, gpu, fold_case, dt, nb, form):
    """ddl_reduce_fold; ddl_reduce_fold_ordered with orders 1 and 2 (fp16 / bf16 keep the fp32 left
    fold); the run form (config fold_form 2); buffers one element off alignment (k_sumN_scalar); and
    ddl_reduce_fold_batch with the set split into two problems of unequal, odd lengths."""
    xs, want = fold_case(dt, nb)
    n = xs[0].size
    P = VP * nb
    if form == 'offset':
        sx, so = [_Shifted(x, gpu) for x in xs], _Shifted(xs[0], gpu, fill=False)
        _ok(lib, lib.ddl_reduce_fold(so.ptr, sx[0].ptr, P(*[s.ptr for s in sx[1:]]), nb, n, dt, _stream()))
        assert_same(dt, so.result().view(NP[dt]), want, f'{NAME[dt]} nb={nb} offset')
        return
    if form == 'batch':
        cut = 655_387  # odd: both problems end in a partial vector, and both start on aligned buffers
        parts = [[to_dev(x[:cut], gpu) for x in xs], [to_dev(x[cut:], gpu) for x in xs]]
        outs = [torch.zeros_like(p[0]) for p in parts]
        O, A = (VP * 2)(*[o.data_ptr() for o in outs]), (VP * 2)(*[p[0].data_ptr() for p in parts])
        B = (VP * (2 * nb))(*[t.data_ptr() for p in parts for t in p[1:]])
        st = lib.ddl_reduce_fold_batch(2, O, A, B, nb, (SZ * 2)(cut, n - cut), dt, 0, _stream())
        _ok(lib, st)
        got = np.concatenate([to_host(o, dt) for o in outs])
        assert_same(dt, got, want, f'{NAME[dt]} nb={nb} batch')
        return
    ts = [to_dev(x, gpu) for x in xs]
    out = torch.zeros_like(ts[0])
    ins = P(*[t.data_ptr() for t in ts[1:]])
    if form == 'fold':
        st = lib.ddl_reduce_fold(out.data_ptr(), ts[0].data_ptr(), ins, nb, n, dt, _stream())
    elif form == 'run_form':
        with config(lib, fold_form=2):
            st = lib.ddl_reduce_fold(out.data_ptr(), ts[0].data_ptr(), ins, nb, n, dt, _stream())
    else:
        order = {'ordered1': 1, 'ordered2': 2}[form]
        st = lib.ddl_reduce_fold_ordered(out.data_ptr(), ts[0].data_ptr(), ins, nb, n, dt, order, _stream())
    _ok(lib, st)
    assert_same(dt, to_host(out, dt), want, f'{NAME[dt]} nb={nb} {form}')


# ---- fp32 / fp64: the edge table -------------------------------------------------------------------
@pytest.mark.parametrize('offset', [False, True], ids=['aligned', 'offset'])
@pytest.mark.parametrize('dt', eh.FLOAT_TYPES, **BY_NAME)
def test_float_edge_table(lib, oracle, gpu, dt, offset):
    """E x E (zeros, subnormals, tiny, max, inf, NaN, ...) through ddl_reduce_sum2, ddl_reduce_fold with
    nb = 2 (the third input is the table reversed) and ddl_reduce_fold_ordered order 1, against numpy's
    `+` and the oracle's MPICH order."""
    a, b = eh.edge_table(dt)
    c = b[::-1].copy()
    n = a.size
    P = VP * 2

    def dev(x, fill=True):
        if offset:
            return _Shifted(x, gpu, fill)
        return to_dev(x if fill else np.zeros_like(x), gpu)

    def ptr(t):
        return t.ptr if offset else t.data_ptr()

    def host(t):
        return t.result() if offset else to_host(t, dt)

    ta, tb, tc = dev(a), dev(b), dev(c)
    out = dev(a, fill=False)
    _ok(lib, lib.ddl_reduce_sum2(ptr(out), ptr(ta), ptr(tb), n, dt, _stream()))
    assert_same(dt, host(out), eh.np_add([a, b]), f'{NAME[dt]} sum2')
    out = dev(a, fill=False)
    _ok(lib, lib.ddl_reduce_fold(ptr(out), ptr(ta), P(ptr(tb), ptr(tc)), 2, n, dt, _stream()))
    assert_same(dt, host(out), eh.np_add([a, b, c]), f'{NAME[dt]} fold')
    out = dev(a, fill=False)
    _ok(lib, lib.ddl_reduce_fold_ordered(ptr(out), ptr(ta), P(ptr(tb), ptr(tc)), 2, n, dt, 1, _stream()))
    assert_same(dt, host(out), oracle.fold_ref_order(dt, [a, b, c], 4096), f'{NAME[dt]} fold, MPICH order')


# ---- the converting pack ----------------------------------------------------------------------------
@pytest.mark.parametrize('aligned', [True, False], ids=['vector', 'elements'])
@pytest.mark.parametrize('wire', eh.HALF_TYPES, ids=lambda d: WIRE_NAME[d])
def test_pack_every_wire_pattern(lib, gpu, wire, aligned):
    """The pack set (every finite wire pattern's value, the exact midpoint to the next one and its two
    fp32 neighbours, ±inf, NaNs with the payload in the low bits only) as one segment through
    ddl_pack_cvt, from a 16-byte-aligned tensor and from one that is only 4-byte aligned."""
    x = eh.pack_set(wire)
    n = x.size
    lead = 64 if aligned else 68
    host = np.full(lead + x.nbytes + 64, GUARD, np.uint8)
    host[lead:lead + x.nbytes] = x.view(np.uint8)
    src = torch.from_numpy(host).to(gpu)
    assert (src.data_ptr() + lead) % 16 == (0 if aligned else 4)
    pad = 256
    flat = torch.full((pad + (2 * n + 255) // 256 * 256 + pad,), GUARD, dtype=torch.uint8, device=gpu)
    st = lib.ddl_pack_cvt(flat.data_ptr() + pad, (VP * 1)(src.data_ptr() + lead), (SZ * 1)(n), 1, wire, _stream())
    _ok(lib, st)
    got = flat.cpu().numpy()
    want = narrow(wire, x)
    assert_same(wire, got[pad:pad + 2 * n].view(want.dtype), want, f'{WIRE_NAME[wire]}')
    assert (got[:pad] == GUARD).all() and (got[pad + 2 * n:] == GUARD).all(), 'bytes around the segment were written'
    assert src.cpu().numpy().tobytes() == host.tobytes(), 'the pack wrote to its source'


# ---- one schedule-level check per type ---------------------------------------------------------------
def _local_allreduce(lib, gpu, xs, dt):
    ins = [to_dev(x, gpu) for x in xs]
    outs = [torch.zeros_like(t) for t in ins]
    P = len(xs)
    st = lib.ddl_local_ring_allreduce(P, (VP * P)(*[t.data_ptr() for t in ins]), (VP * P)(*[t.data_ptr() for t in outs]),
                                      xs[0].size, dt, 0, _stream())
    _ok(lib, st)
    return [to_host(o, dt) for o in outs]


@pytest.mark.parametrize('schedule', ['ring', 'direct'])
@pytest.mark.parametrize('dt', eh.HALF_TYPES, **BY_NAME)
def test_schedules_every_pattern(lib, oracle, gpu, dt, schedule):
    """x_0, x_1, x_2 of the fold set as three ranks: the ring (one rounding per hop, the rings the
    engine reports) and the direct schedule (fp32 fold, one rounding), in their own orders."""
    xs = eh.fold_set(dt, 2)
    n = xs[0].size
    if schedule == 'ring':
        with config(lib, reference_order=0, algo=0):
            outs = _local_allreduce(lib, gpu, xs, dt)
            R, _ = ring_shape(lib, n, dt, 3)
            want = oracle.allreduce_ring(dt, xs, ring_perms(lib, 3, R))
    else:
        with config(lib, reference_order=0, algo=1):
            outs = _local_allreduce(lib, gpu, xs, dt)
        want = oracle.allreduce_direct(dt, xs)
    for r, o in enumerate(outs):
        assert_same(dt, o, want, f'{NAME[dt]} {schedule} rank {r}')
