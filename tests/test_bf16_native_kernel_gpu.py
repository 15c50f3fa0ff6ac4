"""The native bfloat16 scaled and counted fusion copies (csrc/pack.hip: ScaleGather16Op, DivOp<kDivBF16, true>,
k_seg_sumsq16) on their own, through ddl_pack_scale_dtype / ddl_unpack_scale_dtype / ddl_unpack_ops_sumsq, bit
for bit against the NumPy model (_bf16_native_helpers.py). A NaN must be a NaN (its payload is free); nothing
outside the segments may change; a launch with every factor 1 and nothing wanted is the plain kernels'."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _bf16_native_helpers as bh
from _bf16_native_helpers import ALL_BITS, OP_AVG, OP_SUM, THIRD, THREE, assert_same, same_double
from _scale_helpers import LENS

pytestmark = pytest.mark.gpu
GUARD = 0xA5
DT_BFLOAT16, DT_HALF, DT_DOUBLE = 14, 19, 2
UNSUPPORTED_DTYPE = 4
P = 3
MISALIGNED = {LENS.index(4099)}  # the tensor at a 2-byte-offset address
BIG = 4096 * 512 + 7             # more than 4096 tiles: the finish takes its second level


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _round256(b):
    return (b + 255) & ~255


def _layout(lens, misaligned):
    offs, cur = [], 64
    for i, n in enumerate(lens):
        cur = (cur + 15) & ~15
        if i in misaligned:
            cur += 2
        offs.append(cur)
        cur += 2 * n + (48 if n else 0)  # guard bytes after every non-empty segment
    return offs, cur + 64


def _floats(values):
    return (ctypes.c_float * len(values))(*[float(v) for v in values])


def _pack(lib, gpu, xs, scale=None, misaligned=()):
    """Gather the bf16 segments xs into a 0x5A-filled flat buffer; scale None: ddl_pack. Returns its bytes."""
    k, lens = len(xs), [len(x) for x in xs]
    offs, total = _layout(lens, misaligned)
    host = np.full(total, GUARD, np.uint8)
    for x, o in zip(xs, offs):
        host[o:o + 2 * len(x)] = x.view(np.uint8)
    src = torch.from_numpy(host).to(gpu)
    flat = torch.full((max(256, sum(_round256(2 * n) for n in lens)),), 0x5A, dtype=torch.uint8, device=gpu)
    srcs = (ctypes.c_void_p * k)(*[src.data_ptr() + o for o in offs])
    if scale is not None:
        st = lib.ddl_pack_scale_dtype(flat.data_ptr(), srcs, (ctypes.c_size_t * k)(*lens), k, DT_BFLOAT16, _floats(scale),
                                      _stream())
    else:
        st = lib.ddl_pack(flat.data_ptr(), srcs, (ctypes.c_size_t * k)(*[2 * n for n in lens]), k, _stream())
    assert st == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    assert src.cpu().numpy().tobytes() == host.tobytes(), 'a pack wrote to its sources'
    return flat.cpu().numpy()


def _unpack(lib, gpu, data, ops, scale=None, want=None, misaligned=(), in_place=False, stat_only=False):
    """Scatter the flat side's bf16 contents `data` into guarded tensors (in_place: the tensors hold them).
    scale None: ddl_unpack_ops / ddl_unpack_ops_sumsq. Returns (segments as uint16, sums of squares or None)."""
    k, lens = len(data), [len(x) for x in data]
    flat = np.full(max(256, sum(_round256(2 * n) for n in lens)), 0x5A, np.uint8)
    off = 0
    for x in ([] if in_place else data):
        flat[off:off + x.nbytes] = x.view(np.uint8)
        off += _round256(x.nbytes)
    offs, total = _layout(lens, misaligned)
    host = np.full(total, GUARD, np.uint8)
    if in_place:
        for x, o in zip(data, offs):
            host[o:o + 2 * len(x)] = x.view(np.uint8)
    dst = torch.from_numpy(host).to(gpu)
    src = torch.from_numpy(flat).to(gpu)
    dsts = (ctypes.c_void_p * k)(*[dst.data_ptr() + o for o in offs])
    cops = (ctypes.c_int * k)(*ops)
    sp = None if in_place else src.data_ptr()
    out = (ctypes.c_double * k)(*([-1.0] * k))
    cw = (ctypes.c_ubyte * k)(*want) if want is not None else None
    elems = (ctypes.c_size_t * k)(*lens)
    sizes = (ctypes.c_size_t * k)(*[2 * n for n in lens])
    if scale is not None:
        st = lib.ddl_unpack_scale_dtype(dsts, sp, elems, cops, k, DT_BFLOAT16, P, _floats(scale), _stream(), cw,
                                        out if want is not None else None)
    elif want is None:
        st = lib.ddl_unpack_ops(dsts, sp, sizes, cops, k, DT_BFLOAT16, P, _stream())
    else:
        st = lib.ddl_unpack_ops_sumsq(dsts, sp, sizes, cops, k, DT_BFLOAT16, P, _stream(), cw, out)
    assert st == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    covered = np.zeros(got.size, bool)
    for o, n in zip(offs, lens):
        covered[o:o + 2 * n] = True
    assert (got[~covered] == GUARD).all(), 'bytes outside the segments were written'
    if stat_only:
        assert got.tobytes() == host.tobytes(), 'the read-only statistic wrote'
    assert src.cpu().numpy().tobytes() == flat.tobytes(), 'an unpack wrote to the flat buffer'
    return [got[o:o + 2 * n].view(np.uint16) for o, n in zip(offs, lens)], (list(out) if want is not None else None)


def _inputs(seed, lens=LENS):
    return [bh.native_input(n, seed + i) for i, n in enumerate(lens)]


def test_scaled_pack(lib, gpu):
    """c = narrow(widen(g) (x) a) per segment, the factors mixed with 1 among them; a factor-1 segment and the
    padding between the segments have the plain pack's bytes."""
    for shift in (0, 1, 2):
        fs = bh.mixed_factors(len(LENS), shift)
        assert any(f == 1 and n for f, n in zip(fs, LENS)) and any(f != 1 and n for f, n in zip(fs, LENS))
        xs = _inputs(100 * shift)
        got = _pack(lib, gpu, xs, fs, MISALIGNED)
        plain = _pack(lib, gpu, xs, None, MISALIGNED)
        off = 0
        for i, (x, f) in enumerate(zip(xs, fs)):
            assert_same(got[off:off + 2 * len(x)].view(np.uint16), bh.pack(x, f), f'shift {shift} segment {i}')
            if f == 1:
                assert got[off:off + 2 * len(x)].tobytes() == plain[off:off + 2 * len(x)].tobytes() == x.tobytes()
            pad = slice(off + 2 * len(x), off + _round256(2 * len(x)))
            assert (got[pad] == 0x5A).all(), 'padding between segments was written'
            off += _round256(2 * len(x))


@pytest.mark.parametrize('in_place', [False, True], ids=['scatter', 'in_place'])
def test_scaled_unpack(lib, gpu, in_place):
    """SUM and AVG mixed at P = 3, the factors mixed: narrow(widen(s) (/) P (x) b), one rounding; in place the
    same bits from one launch, a SUM segment with factor 1 untouched."""
    seen = set()
    for shift in (0, 2, 3):
        fs = bh.mixed_factors(len(LENS), shift + 1)
        ops = [OP_AVG if (i + shift) % 3 else OP_SUM for i in range(len(LENS))]
        seen |= {(o, bool(f == 1), i in MISALIGNED) for i, (o, f, n) in enumerate(zip(ops, fs, LENS)) if n}
        data = _inputs(300 + shift)
        got, _ = _unpack(lib, gpu, data, ops, fs, misaligned=MISALIGNED, in_place=in_place)
        plain, _ = _unpack(lib, gpu, data, ops, None, misaligned=MISALIGNED, in_place=in_place)
        for i, (s, g, p, f) in enumerate(zip(data, got, plain, fs)):
            assert_same(g, bh.unpack(s, ops[i], P, f), f'shift {shift} segment {i} op {ops[i]} factor {f}')
            if f == 1:
                assert g.tobytes() == p.tobytes(), 'a factor-1 segment differs from the plain kernel'
                if ops[i] == OP_SUM:
                    assert g.tobytes() == s.tobytes()
    # every kind of segment was in some launch; the 2-byte-aligned tensor as SUM and as AVG with a factor
    assert {(o, one) for o, one, _ in seen} == {(OP_SUM, True), (OP_SUM, False), (OP_AVG, True), (OP_AVG, False)}
    assert {(OP_SUM, False, True), (OP_AVG, False, True)} <= seen


def test_unpack_with_the_statistic(lib, gpu):
    """The counted scatter stores the scaled scatter's bytes; a wanted segment's double is the 2-byte layout's
    order over widen(stored), an unwanted one's +0.0; with and without factors in the launch."""
    for fs in (bh.mixed_factors(len(LENS), 1), None):
        ops = [OP_AVG if i % 2 else OP_SUM for i in range(len(LENS))]
        want = [0 if i % 3 == 2 else 1 for i in range(len(LENS))]
        for data in (_inputs(500), [bh.native_input(n, 600 + i, specials=False) for i, n in enumerate(LENS)]):
            ref, _ = _unpack(lib, gpu, data, ops, fs, misaligned=MISALIGNED)
            got, sq = _unpack(lib, gpu, data, ops, fs, want=want, misaligned=MISALIGNED)
            for i, (s, g, r) in enumerate(zip(data, got, ref)):
                assert_same(g, bh.unpack(s, ops[i], P, fs[i] if fs else 1.0), f'segment {i}')
                assert_same(g, r)
                m = bh.sumsq(g) if want[i] else 0.0
                assert same_double(sq[i], m), (i, sq[i], m)
            # the read-only in-place form over the results: the same doubles, nothing written
            _, sq2 = _unpack(lib, gpu, got, ops, None, want=want, misaligned=MISALIGNED, in_place=True, stat_only=True)
            assert all(same_double(a, b) for a, b in zip(sq, sq2)), (sq, sq2)
    assert all(math.isfinite(v) for v in sq)  # (the last data set holds finite values only)


def test_every_bf16_pattern(lib, gpu):
    """All 65 536 patterns: the pack with a = 1/3 (a truncating narrow differs on 21 926 of them), the unpack
    with AVG at P = 3 and b = 1/3 (a rounding between quotient and factor: 13 584), b = 3 (the factor ahead
    of the quotient: 426), SUM with b = 1/3, and the plain bytes with b = 1."""
    got = _pack(lib, gpu, [ALL_BITS, ALL_BITS], [THIRD, 1.0], misaligned={1})
    assert_same(got[:2 * 65536].view(np.uint16), bh.pack(ALL_BITS, THIRD), 'pack a = 1/3')
    assert got[2 * 65536:4 * 65536].tobytes() == ALL_BITS.tobytes()
    data, ops, fs = [ALL_BITS] * 5, [OP_AVG, OP_AVG, OP_SUM, OP_SUM, OP_AVG], [THIRD, THREE, THIRD, 1.0, 1.0]
    for in_place in (False, True):
        out, _ = _unpack(lib, gpu, data, ops, fs, misaligned={1}, in_place=in_place)
        for i, g in enumerate(out):
            assert_same(g, bh.unpack(ALL_BITS, ops[i], P, fs[i]), f'pattern unpack {i} in_place {in_place}')
        assert out[3].tobytes() == ALL_BITS.tobytes()
    out, sq = _unpack(lib, gpu, data, ops, fs, want=[1] * 5, misaligned={1})
    for i, g in enumerate(out):
        assert_same(g, bh.unpack(ALL_BITS, ops[i], P, fs[i]), f'pattern sumsq unpack {i}')
        assert math.isnan(sq[i])
    fin = ALL_BITS[np.isfinite(bh.wide(ALL_BITS))]
    out, sq = _unpack(lib, gpu, [fin] * 3, [OP_AVG, OP_SUM, OP_SUM], [THIRD, THREE, 1.0], want=[1, 1, 1])
    for i, g in enumerate(out):
        m = bh.sumsq(g)
        assert same_double(sq[i], m), (i, sq[i], m)
    # finite exactly when every STORED element is: 3 x the largest values overflows in the narrowing
    assert math.isfinite(sq[0]) and math.isinf(sq[1]) and math.isfinite(sq[2])


def test_long_segment_takes_the_second_finish_level(lib, gpu):
    x = bh.native_input(BIG, 77, specials=False)
    out, sq = _unpack(lib, gpu, [x, x[:300]], [OP_AVG, OP_SUM], [THIRD, 1.0], want=[1, 1], misaligned={0})
    assert_same(out[0], bh.unpack(x, OP_AVG, P, THIRD))
    m = bh.sumsq(out[0])
    assert math.isfinite(m) and same_double(sq[0], m), (sq[0], m)
    assert same_double(sq[1], bh.sumsq(x[:300]))


def test_all_factors_one_nothing_wanted_is_the_plain_launch(lib, gpu):
    xs = _inputs(7)
    ones = [1.0] * len(LENS)
    assert _pack(lib, gpu, xs, ones, MISALIGNED).tobytes() == _pack(lib, gpu, xs, None, MISALIGNED).tobytes()
    ops = [OP_AVG if i % 2 else OP_SUM for i in range(len(LENS))]
    for in_place in (False, True):
        got, _ = _unpack(lib, gpu, xs, ops, ones, misaligned=MISALIGNED, in_place=in_place)
        ref, _ = _unpack(lib, gpu, xs, ops, None, misaligned=MISALIGNED, in_place=in_place)
        assert all(g.tobytes() == r.tobytes() for g, r in zip(got, ref))
    got, sq = _unpack(lib, gpu, xs, ops, ones, want=[0] * len(LENS), misaligned=MISALIGNED)
    assert all(g.tobytes() == r.tobytes() for g, r in zip(got, ref)) and sq == [0.0] * len(LENS)


def test_other_dtypes_and_bad_factors_are_refused(lib, gpu):
    t = torch.zeros(64, dtype=torch.int16, device=gpu)
    flat = torch.zeros(256, dtype=torch.uint8, device=gpu)
    one = (ctypes.c_void_p * 1)(t.data_ptr())
    n8, sum_op, want = (ctypes.c_size_t * 1)(8), (ctypes.c_int * 1)(OP_SUM), (ctypes.c_ubyte * 1)(1)
    out = (ctypes.c_double * 1)()
    for dt in (DT_HALF, DT_DOUBLE):
        assert lib.ddl_pack_scale_dtype(flat.data_ptr(), one, n8, 1, dt, _floats([0.5]), _stream()) == UNSUPPORTED_DTYPE
        assert lib.ddl_unpack_scale_dtype(one, flat.data_ptr(), n8, sum_op, 1, dt, P, _floats([0.5]), _stream(), None,
                                          None) == UNSUPPORTED_DTYPE
        assert lib.ddl_unpack_scale_dtype(one, flat.data_ptr(), n8, sum_op, 1, dt, P, _floats([1.0]), _stream(), want,
                                          out) == UNSUPPORTED_DTYPE
        assert lib.ddl_unpack_ops_sumsq(one, flat.data_ptr(), (ctypes.c_size_t * 1)(16), sum_op, 1, dt, P, _stream(), want,
                                        out) == UNSUPPORTED_DTYPE
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        assert lib.ddl_pack_scale_dtype(flat.data_ptr(), one, n8, 1, DT_BFLOAT16, _floats([bad]), _stream()) == 3, bad
    torch.cuda.synchronize()
    assert not t.any() and not flat.any()  # nothing ran
    got = _pack(lib, gpu, [np.full(8, 0x4040, np.uint16)], [0.5])
    assert got[:16].view(np.uint16).tolist() == [0x3fc0] * 8
