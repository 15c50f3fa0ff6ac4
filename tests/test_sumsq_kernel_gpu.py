"""The unpack kernels with the sum of squares (csrc/pack.hip k_seg_sumsq + k_sumsq_finish) on their own,
through ddl_unpack_ops_sumsq / ddl_unpack_cvt_sumsq.

What they store must be what ddl_unpack_ops / ddl_unpack_cvt store for the same inputs, byte for byte;
every sum of squares must be, bit for bit, the NumPy restatement of the documented order
(_sumsq_helpers.mirror) over the values that were stored. A NaN must be a NaN (its payload is free)."""
import ctypes
import math
import struct

import numpy as np
import pytest
import torch

from _sumsq_helpers import mirror

pytestmark = pytest.mark.gpu
GUARD = 0xA5
DT_FLOAT, DT_BFLOAT16, DT_HALF = 1, 14, 19
OP_SUM, OP_AVG = 0, 1
P = 3
# the tile edges of both forms (256 / 512 elements), more than 64 tiles (the finishing kernel's strided
# loop: 16385 elements are 65 tiles of 256, 70_001 are 137 tiles of 512), then a run of 300 empty
# segments between two non-empty ones (more than 255 segments in one index block: the int32 tile index)
LENS = [0, 1, 3, 4, 5, 255, 256, 257, 511, 512, 513, 16383, 16384, 16385, 70_001] + [0] * 300 + [9, 515]
MISALIGNED = {LENS.index(5), LENS.index(256), LENS.index(513), LENS.index(16385), LENS.index(70_001), len(LENS) - 1}
TORCH_WIRE = {DT_HALF: torch.float16, DT_BFLOAT16: torch.bfloat16}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _round256(b):
    return (b + 255) & ~255


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) or struct.pack('<d', a) == struct.pack('<d', b)


def _wire_bits(x, wire):
    """fp32 values rounded to the wire type, as uint16 bit patterns."""
    return torch.from_numpy(np.ascontiguousarray(x)).to(TORCH_WIRE[wire]).view(torch.int16).numpy().view(np.uint16)


def _layout(lens, misaligned):
    offs, cur = [], 64
    for i, n in enumerate(lens):
        cur = (cur + 15) & ~15
        if i in misaligned:
            cur += 4
        offs.append(cur)
        cur += 4 * n + (48 if n else 0)  # guard bytes after every non-empty segment
    return offs, cur + 64


def _run(lib, gpu, data, wire, ops, want, misaligned=(), in_place=False, reference=False):
    """`data`: per segment the flat side's contents (fp32 values, or uint16 wire bit patterns with
    `wire`). Returns (the destination bytes, the segments' byte offsets, the sums of squares). In place
    the destination starts as the fp32 `data`. `reference`: ddl_unpack_ops / ddl_unpack_cvt instead."""
    k = len(data)
    lens = [len(x) for x in data]
    es = 2 if wire else 4
    flat = np.full(max(256, sum(_round256(n * es) for n in lens)), 0x5A, np.uint8)
    off = 0
    for x in ([] if in_place else data):
        flat[off:off + x.nbytes] = x.view(np.uint8)
        off += _round256(x.nbytes)
    offs, total = _layout(lens, misaligned)
    host = np.full(total, GUARD, np.uint8)
    if in_place:
        for x, o in zip(data, offs):
            host[o:o + 4 * len(x)] = x.astype(np.float32).view(np.uint8)
    dst = torch.from_numpy(host).to(gpu)
    src = torch.from_numpy(flat).to(gpu)
    dsts = (ctypes.c_void_p * k)(*[dst.data_ptr() + o for o in offs])
    sizes = (ctypes.c_size_t * k)(*[n if wire else 4 * n for n in lens])
    cops = (ctypes.c_int * k)(*ops)
    sp = None if in_place else src.data_ptr()
    out = (ctypes.c_double * k)(*([-1.0] * k))
    if reference:
        fn = lib.ddl_unpack_cvt if wire else lib.ddl_unpack_ops
        st = fn(dsts, sp, sizes, cops, k, wire if wire else DT_FLOAT, P, _stream())
    else:
        fn = lib.ddl_unpack_cvt_sumsq if wire else lib.ddl_unpack_ops_sumsq
        st = fn(dsts, sp, sizes, cops, k, wire if wire else DT_FLOAT, P, _stream(), (ctypes.c_ubyte * k)(*want), out)
    assert st == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    return dst.cpu().numpy(), offs, list(out)


def _segments(got, offs, lens):
    return [got[o:o + 4 * n].view(np.float32) for o, n in zip(offs, lens)]


def _random(lens, wire, seed):
    rng = np.random.default_rng(seed)
    xs = [(rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4)).astype(np.float32) for n in lens]
    return [_wire_bits(x, wire) for x in xs] if wire else xs


@pytest.mark.parametrize('wire', [0, DT_HALF, DT_BFLOAT16], ids=['fp32', 'fp16', 'bf16'])
def test_geometry(lib, gpu, wire):
    """SUM and AVG segments at P = 3, wanted and unwanted mixed: the stored bytes are the plain kernels',
    the guard bytes are untouched, every wanted value is the mirror's and every unwanted one +0.0."""
    lens = LENS
    data = _random(lens, wire, 77)
    nonempty = [i for i, n in enumerate(lens) if n]
    ops = [OP_AVG if (nonempty.index(i) if n else i) % 2 == 1 else OP_SUM for i, n in enumerate(lens)]
    want = [0 if i % 3 == 2 else 1 for i in range(len(lens))]
    assert {(ops[i], want[i]) for i in nonempty} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    ref, offs, _ = _run(lib, gpu, data, wire, ops, want, MISALIGNED, reference=True)
    got, offs2, sq = _run(lib, gpu, data, wire, ops, want, MISALIGNED)
    assert offs == offs2
    assert got.tobytes() == ref.tobytes(), 'stored bytes differ from the unpack without the statistic'
    covered = np.zeros(got.size, bool)
    for o, n in zip(offs, lens):
        covered[o:o + 4 * n] = True
    assert (got[~covered] == GUARD).all(), 'bytes outside the segments were written'
    for i, seg in enumerate(_segments(got, offs, lens)):
        if want[i]:
            m = mirror(seg, bool(wire))
            assert same(sq[i], m), (i, lens[i], sq[i], m)
        else:
            assert struct.pack('<d', sq[i]) == struct.pack('<d', 0.0), (i, sq[i])


@pytest.mark.parametrize('wire', [0, DT_BFLOAT16], ids=['fp32', 'bf16'])
def test_invariance_and_sharing(lib, gpu, wire):
    """The same data gives the same double as an aligned segment, as a misaligned one and in place
    (aligned and misaligned), alone in the launch or among other segments."""
    for n in (5, 513, 16385, 70_001):
        x = _random([n], wire, 1000 + n)[0]
        vals = torch.from_numpy(x.view(np.int16)).view(TORCH_WIRE[wire]).float().numpy() if wire else x
        expect = mirror(vals, bool(wire))
        assert math.isfinite(expect) and expect > 0
        others = _random([300, 1, 4099], wire, 5)
        forms = {}
        forms['aligned'] = _run(lib, gpu, [x], wire, [OP_SUM], [1])[2][0]
        forms['misaligned'] = _run(lib, gpu, [x], wire, [OP_SUM], [1], misaligned={0})[2][0]
        forms['in place'] = _run(lib, gpu, [vals], wire, [OP_SUM], [1], in_place=True)[2][0]
        forms['in place misaligned'] = _run(lib, gpu, [vals], wire, [OP_SUM], [1], misaligned={0}, in_place=True)[2][0]
        shared = [others[0], others[1], x, others[2]]
        forms['shared'] = _run(lib, gpu, shared, wire, [OP_AVG, OP_SUM, OP_SUM, OP_AVG], [1, 0, 1, 1], misaligned={1})[2][2]
        forms['shared unwanted neighbours'] = _run(lib, gpu, shared, wire, [OP_SUM] * 4, [0, 0, 1, 0], misaligned={2})[2][2]
        for name, v in forms.items():
            assert same(v, expect), (n, name, v, expect)


@pytest.mark.parametrize('wire', [0, DT_BFLOAT16], ids=['fp32', 'bf16'])
def test_more_than_4096_tiles(lib, gpu, wire):
    """Segments of more than 4096 tiles (the finishing reduction's second level) beside short ones, flat
    to tensors and in place; one element past a group of 4096 tiles, and several groups."""
    per_tile = 512 if wire else 256
    lens = [300, 4096 * per_tile + 1, 5, 3 * 4096 * per_tile + 70_001, 4096 * per_tile]
    data = _random(lens, wire, 4096)
    got, offs, sq = _run(lib, gpu, data, wire, [OP_AVG, OP_SUM, OP_SUM, OP_AVG, OP_SUM], [1] * 5, misaligned={3})
    segs = _segments(got, offs, lens)
    for i, seg in enumerate(segs):
        m = mirror(seg, bool(wire))
        assert math.isfinite(m) and same(sq[i], m), (i, lens[i], sq[i], m)
    _, _, sq2 = _run(lib, gpu, [s.copy() for s in segs], wire, [OP_SUM] * 5, [0, 1, 0, 1, 1], misaligned={1}, in_place=True)
    assert [same(a, b) for a, b in zip(sq2, [0.0, sq[1], 0.0, sq[3], sq[4]])] == [True] * 5, (sq, sq2)


def test_in_place_is_read_only(lib, gpu):
    """src == NULL: nothing is divided or written, also for AVG segments; unwanted segments are not read."""
    data = _random([300, 0, 5000, 17], 0, 9)
    got, offs, sq = _run(lib, gpu, data, 0, [OP_AVG, OP_AVG, OP_SUM, OP_AVG], [1, 1, 1, 0], misaligned={2}, in_place=True)
    for x, seg in zip(data, _segments(got, offs, [len(x) for x in data])):
        assert seg.tobytes() == x.tobytes()
    covered = np.zeros(got.size, bool)
    for o, x in zip(offs, data):
        covered[o:o + x.nbytes] = True
    assert (got[~covered] == GUARD).all()
    assert [same(v, mirror(x, False)) for v, x in zip(sq[:3], data[:3])] == [True] * 3 and sq[3] == 0.0


def test_edge_values(lib, gpu):
    f = np.finfo(np.float32)
    big_sub = np.nextafter(f.tiny, np.float32(0))
    finite = np.array([0.0, -0.0, f.smallest_subnormal, -f.smallest_subnormal, big_sub, -big_sub, f.tiny, f.max, -f.max,
                       1.0, -3.0], np.float32)
    zeros = np.array([0.0, -0.0, -0.0], np.float32)
    cases = {'finite': finite, 'zeros': zeros, 'max': np.full(1000, f.max, np.float32),
             'inf': np.concatenate([finite, [np.inf]]).astype(np.float32),
             '-inf': np.concatenate([[-np.inf], finite]).astype(np.float32),
             'nan': np.concatenate([finite, [np.nan], finite]).astype(np.float32),
             'inf and nan': np.concatenate([[np.inf], finite, [np.nan]]).astype(np.float32)}
    names = list(cases)
    for in_place in (False, True):
        _, _, sq = _run(lib, gpu, [cases[c] for c in names], 0, [OP_SUM] * len(names), [1] * len(names),
                        in_place=in_place)
        got = dict(zip(names, sq))
        for c in names:
            assert same(got[c], mirror(cases[c], False)), (c, got[c])
        assert math.isfinite(got['finite']) and math.isfinite(got['max']) and got['max'] > 1e79
        assert struct.pack('<d', got['zeros']) == struct.pack('<d', 0.0)
        assert got['inf'] == math.inf and got['-inf'] == math.inf
        assert math.isnan(got['nan']) and math.isnan(got['inf and nan'])


@pytest.mark.parametrize('wire', [DT_HALF, DT_BFLOAT16], ids=['fp16', 'bf16'])
def test_every_16_bit_pattern(lib, gpu, wire):
    """All 65536 patterns, split into the finite and the non-finite ones so that the finite part checks
    bits and not just "NaN"; SUM and AVG at P = 3."""
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    vals = torch.from_numpy(bits.view(np.int16)).view(TORCH_WIRE[wire]).float().numpy()
    fin, non = bits[np.isfinite(vals)], bits[~np.isfinite(vals)]
    assert fin.size > 60000 and non.size > 2
    data, ops = [fin, non, fin, non, bits], [OP_SUM, OP_SUM, OP_AVG, OP_AVG, OP_AVG]
    ref, offs, _ = _run(lib, gpu, data, wire, ops, [1] * 5, reference=True)
    got, _, sq = _run(lib, gpu, data, wire, ops, [1] * 5)
    assert got.tobytes() == ref.tobytes()
    segs = _segments(got, offs, [len(x) for x in data])
    for i in (0, 2):
        m = mirror(segs[i], True)
        assert math.isfinite(m) and m > 0 and struct.pack('<d', sq[i]) == struct.pack('<d', m), (i, sq[i], m)
    for i in (1, 3, 4):
        assert math.isnan(sq[i]) and math.isnan(mirror(segs[i], True))
    inf_only = bits[np.isinf(vals)]
    _, _, sq = _run(lib, gpu, [inf_only], wire, [OP_AVG], [1])
    assert sq[0] == math.inf
