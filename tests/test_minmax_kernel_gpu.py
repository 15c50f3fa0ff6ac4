"""The MIN / MAX combine of the reduce and fold kernels (csrc/reduce_kernels.hip) against the numpy
model of tests/_minmax_helpers.py, both ops, every dtype: the two-input reduce at the sizes where
its paths change (vector, tile, tail; out aliasing either input; guard bytes), the N-input fold in
the tile and the run form, the batched fold, the float edge set as all ordered pairs, and every
16-bit pattern against the 16-bit edge values of tests/_edge_helpers.py.

Compared with assert_same: bit for bit where the expected value is no NaN, a NaN where it is one."""
import ctypes

import numpy as np
import pytest
import torch

import _edge_helpers as eh
from _helpers import ALL_DTYPES, DT_DOUBLE, DT_FLOAT, NAME, NP, config
from _minmax_helpers import OP_NAME, OPS, assert_same, edge_pairs, finite_input, model

pytestmark = pytest.mark.gpu
VP, SZ = ctypes.c_void_p, ctypes.c_size_t
GUARD, PAD = 0xA5, 256
BY_NAME = dict(ids=lambda d: NAME[d])
BY_OP = dict(ids=lambda o: OP_NAME[o])
FOLD_NB = [1, 2, 3, 6, 7, 15]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ok(lib, st):
    assert st == 0, lib.ddl_last_error()
    torch.cuda.synchronize()


class _Arena:
    """Arrays on the device inside one allocation filled with a guard byte, each at a 256-byte
    boundary + `shift` bytes with at least 256 guard bytes on either side."""

    def __init__(self, gpu, arrays, shift=0):
        self.spans, off = [], PAD
        for x in arrays:
            self.spans.append((off + shift, x.nbytes, x.dtype))
            off += shift + ((x.nbytes + PAD - 1) // PAD + 1) * PAD
        host = np.full(off + PAD, GUARD, np.uint8)
        for (o, nb, _), x in zip(self.spans, arrays):
            host[o:o + nb] = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
        self.t = torch.from_numpy(host).to(gpu)
        assert self.t.data_ptr() % 256 == 0

    def ptr(self, i):
        return self.t.data_ptr() + self.spans[i][0]

    def read(self):
        """Every array as it is now; every byte outside the arrays must still be the guard."""
        raw = self.t.cpu().numpy()
        mask = np.ones(raw.size, bool)
        out = []
        for o, nb, dtype in self.spans:
            mask[o:o + nb] = False
            out.append(raw[o:o + nb].view(dtype).copy())
        assert (raw[mask] == GUARD).all(), 'bytes outside the buffers were written'
        return out


def _sizes(dt):
    es = np.dtype(NP[dt]).itemsize
    V, T = 16 // es, 2048 // es
    return sorted({0, 1, V - 1, V, V + 1, T - 1, T, T + 1, 70_001})


@pytest.mark.parametrize('op', OPS, **BY_OP)
@pytest.mark.parametrize('dt', ALL_DTYPES, **BY_NAME)
def test_reduce_op2_sizes_aliasing_and_guards(lib, gpu, dt, op):
    """ddl_reduce_op2 at 0, 1, one 16-byte vector -1 / exact / +1, one 2 KiB tile -1 / exact / +1 and
    70 001 elements: out of place, out = a, out = b; inputs unchanged, nothing outside `out` written.
    And all three buffers one element off the 16-byte alignment (the scalar kernel)."""
    for n in _sizes(dt):
        a, b = finite_input(dt, n, 11 * n + dt), finite_input(dt, n, 13 * n + dt + 1)
        want = model(dt, op, [a, b])
        for alias in ('none', 'a', 'b'):
            ar = _Arena(gpu, [a, b, np.zeros(n, NP[dt])])
            o = {'none': 2, 'a': 0, 'b': 1}[alias]
            _ok(lib, lib.ddl_reduce_op2(ar.ptr(o), ar.ptr(0), ar.ptr(1), n, dt, op, _stream()))
            got = ar.read()
            assert_same(dt, got[o], want, f'{NAME[dt]} n={n} out={alias}')
            if alias != 'a':
                assert got[0].tobytes() == a.tobytes()
            if alias != 'b':
                assert got[1].tobytes() == b.tobytes()
    n = 4099
    a, b = finite_input(dt, n, 5), finite_input(dt, n, 6)
    ar = _Arena(gpu, [a, b, np.zeros(n, NP[dt])], shift=np.dtype(NP[dt]).itemsize)
    assert ar.ptr(0) % 16 != 0
    _ok(lib, lib.ddl_reduce_op2(ar.ptr(2), ar.ptr(0), ar.ptr(1), n, dt, op, _stream()))
    assert_same(dt, ar.read()[2], model(dt, op, [a, b]), f'{NAME[dt]} misaligned')


def _fold(lib, gpu, dt, op, xs, alias_a=False, shift=0):
    n, nb = xs[0].size, len(xs) - 1
    ar = _Arena(gpu, list(xs) + [np.zeros(n, NP[dt])], shift=shift)
    ins = (VP * nb)(*[ar.ptr(1 + k) for k in range(nb)])
    o = 0 if alias_a else nb + 1
    _ok(lib, lib.ddl_reduce_fold_op(ar.ptr(o), ar.ptr(0), ins, nb, n, dt, op, _stream()))
    got = ar.read()
    for k in range(1 if alias_a else 0, nb + 1):
        assert got[k].tobytes() == np.ascontiguousarray(xs[k]).tobytes(), f'input {k} changed'
    return got[o]


@pytest.mark.parametrize('op', OPS, **BY_OP)
@pytest.mark.parametrize('dt', ALL_DTYPES, **BY_NAME)
def test_fold_op_tile_and_run_form(lib, gpu, dt, op):
    """ddl_reduce_fold_op with 1, 2, 3, 6, 7 and 15 received inputs in the tile form (fold_form 1) and
    the run form (2), at 3 runs of 16 KiB + 5 elements and at 1 element; out apart from and aliasing
    a; and the element-granular kernel on misaligned buffers."""
    es = np.dtype(NP[dt]).itemsize
    for n in (3 * 16384 // es + 5, 1):
        pool = [finite_input(dt, n, 100 * k + dt + n) for k in range(16)]
        for nb in FOLD_NB:
            xs = pool[:nb + 1]
            want = model(dt, op, xs)
            for form in (1, 2):
                with config(lib, fold_form=form):
                    got = _fold(lib, gpu, dt, op, xs, alias_a=(nb + form) % 2 == 0)
                assert_same(dt, got, want, f'{NAME[dt]} n={n} nb={nb} form={form}')
    xs = [finite_input(dt, 4099, 7 + k) for k in range(4)]
    assert_same(dt, _fold(lib, gpu, dt, op, xs, shift=es), model(dt, op, xs), f'{NAME[dt]} misaligned fold')


@pytest.mark.parametrize('op', OPS, **BY_OP)
@pytest.mark.parametrize('dt', ALL_DTYPES, **BY_NAME)
def test_fold_batch_op_ragged(lib, gpu, dt, op):
    """ddl_reduce_fold_batch_op: 8 problems of different lengths in one launch, one of them empty."""
    elems, nb = [1, 300, 0, 4099, 70_001, 513, 7, 2048], 4
    xs = [[finite_input(dt, max(n, 1), 31 * p + k + dt)[:n] for k in range(nb + 1)] for p, n in enumerate(elems)]
    ar = _Arena(gpu, [x for row in xs for x in row] + [np.zeros(n, NP[dt]) for n in elems])
    P = len(elems)
    A = (VP * P)(*[ar.ptr(p * (nb + 1)) for p in range(P)])
    I = (VP * (P * nb))(*[ar.ptr(p * (nb + 1) + 1 + k) for p in range(P) for k in range(nb)])
    O = (VP * P)(*[ar.ptr(P * (nb + 1) + p) for p in range(P)])
    _ok(lib, lib.ddl_reduce_fold_batch_op(P, O, A, I, nb, (SZ * P)(*elems), dt, op, _stream()))
    got = ar.read()
    for p in range(P):
        assert_same(dt, got[P * (nb + 1) + p], model(dt, op, xs[p]), f'{NAME[dt]} problem {p}')


def test_kernel_entry_points_refuse_other_ops(lib, gpu):
    t = torch.zeros(64, device=gpu)
    one = (VP * 1)(t.data_ptr())
    for bad in (1, 2, 5, -1):
        assert lib.ddl_reduce_op2(t.data_ptr(), t.data_ptr(), t.data_ptr(), 64, DT_FLOAT, bad, _stream()) == 3
        assert lib.ddl_reduce_fold_op(t.data_ptr(), t.data_ptr(), one, 1, 64, DT_FLOAT, bad, _stream()) == 3
    torch.cuda.synchronize()


@pytest.mark.parametrize('op', OPS, **BY_OP)
@pytest.mark.parametrize('dt', [DT_FLOAT, DT_DOUBLE], **BY_NAME)
def test_float_edge_set_all_ordered_pairs(lib, gpu, dt, op):
    """+-0, subnormals, +-1 and its neighbours, +-max, +-inf and quiet / signalling / negative NaNs as
    all ordered pairs, through the reduce and through a 3-input fold (the third input: the pairs'
    first operand in reverse)."""
    a, b = edge_pairs(dt)
    ar = _Arena(gpu, [a, b, np.zeros(a.size, NP[dt])])
    _ok(lib, lib.ddl_reduce_op2(ar.ptr(2), ar.ptr(0), ar.ptr(1), a.size, dt, op, _stream()))
    assert_same(dt, ar.read()[2], model(dt, op, [a, b]), 'reduce')
    c = np.ascontiguousarray(a[::-1])
    for form in (1, 2):
        with config(lib, fold_form=form):
            assert_same(dt, _fold(lib, gpu, dt, op, [a, b, c]), model(dt, op, [a, b, c]), f'fold form {form}')


@pytest.fixture(scope='module')
def pattern_case():
    """dt -> (every 16-bit pattern tiled once per edge value, the edge values repeated, a third input)."""
    out = {}
    for dt in eh.HALF_TYPES:
        fixed = np.array(eh.FIXED[dt], np.uint16)
        a = np.tile(eh.patterns(), fixed.size)
        b = np.repeat(fixed, eh.N_PATTERNS)
        c = np.repeat(np.roll(fixed, 5), eh.N_PATTERNS)
        out[dt] = tuple(eh.storage(dt, x) for x in (a, b, c))
    return out


@pytest.mark.parametrize('op', OPS, **BY_OP)
@pytest.mark.parametrize('dt', eh.HALF_TYPES, **BY_NAME)
def test_every_16_bit_pattern(lib, gpu, pattern_case, dt, op):
    """All 65 536 patterns against each of the 21 edge values of the type, through the reduce and
    through a 3-input fold in both forms."""
    a, b, c = pattern_case[dt]
    n = a.size
    ta, tb, tc = (torch.from_numpy(np.array(x).view(np.int16)).to(gpu) for x in (a, b, c))
    to = torch.zeros_like(ta)
    _ok(lib, lib.ddl_reduce_op2(to.data_ptr(), ta.data_ptr(), tb.data_ptr(), n, dt, op, _stream()))
    assert_same(dt, to.cpu().numpy().view(NP[dt]), model(dt, op, [a, b]), 'reduce')
    want = model(dt, op, [a, b, c])
    ins = (VP * 2)(tb.data_ptr(), tc.data_ptr())
    for form in (1, 2):
        to.zero_()
        with config(lib, fold_form=form):
            _ok(lib, lib.ddl_reduce_fold_op(to.data_ptr(), ta.data_ptr(), ins, 2, n, dt, op, _stream()))
        assert_same(dt, to.cpu().numpy().view(NP[dt]), want, f'fold form {form}')
