"""The scaled fusion copies (csrc/pack.hip: ScaleGatherOp and the SCALE instances of CvtPackOp, DivOp,
CvtUnpackOp and k_seg_sumsq) on their own, through ddl_pack_scale / ddl_unpack_scale.

A scaled pack must write what the UNSCALED pack writes for inputs multiplied in NumPy; a scaled unpack
what NumPy makes of the unscaled unpack's output; a segment with factor 1 inside a scaled launch the plain
kernel's bytes; nothing outside the segments may change. A NaN must be a NaN (its payload is free)."""
import ctypes
import math
import struct

import numpy as np
import pytest
import torch

from _scale_helpers import (FACTORS, LENS, MISALIGNED, OP_AVG, OP_SUM, mixed_factors, mul, pack_feedback, same_bits,
                            scale_input)
from _sumsq_helpers import mirror
from _wire_helpers import narrow, widen

pytestmark = pytest.mark.gpu
GUARD = 0xA5
DT_FLOAT, DT_BFLOAT16, DT_HALF = 1, 14, 19
WIRES = [0, DT_HALF, DT_BFLOAT16]
WIRE_IDS = ['fp32', 'fp16', 'bf16']
P = 3
THIRD = np.float32(1.0 / 3.0)
# (element counts, segments on a pointer that is only 4-byte aligned, shift of the factors, segments
# without a residual in the feedback test). wide_map, as in test_wire_kernel_gpu.py: more than 255 empty
# segments inside one 128-tile index block, so the int32 tile map (the NARROW = false instances); its
# shift deals a factor of 1 to one of its four non-empty segments at every shift the tests use.
WIDE = [3000, 17] + [0] * 300 + [5, 2048]
GEOMETRIES = {'edges': (LENS, MISALIGNED, 0, {1, 4, 7}), 'wide_map': (WIDE, {1}, 3, {1, 303})}


def _cases(wires, ids):
    """Every wire on every geometry; the 'edges' cases keep the wire alone as their id."""
    return pytest.mark.parametrize('wire,geo', [(w, g) for g in GEOMETRIES for w in wires],
                                   ids=[i if g == 'edges' else f'{i}-{g}' for g in GEOMETRIES for i in ids])


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _round256(b):
    return (b + 255) & ~255


def _layout(lens, misaligned):
    offs, cur = [], 64
    for i, n in enumerate(lens):
        cur = (cur + 15) & ~15
        if i in misaligned:
            cur += 4
        offs.append(cur)
        cur += 4 * n + (48 if n else 0)  # guard bytes after every non-empty segment
    return offs, cur + 64


def _floats(k, values):
    return (ctypes.c_float * k)(*[float(v) for v in values])


def _flat_values(flat, wire):
    """The flat buffer's contents as fp32 (the wire values widened), for a comparison that frees NaN payloads."""
    return widen(wire, flat.view(np.float16 if wire == DT_HALF else np.uint16)) if wire else flat.view(np.float32)


def _pack(lib, gpu, xs, wire, scale=None, residuals=None, misaligned=()):
    """Gather the fp32 segments xs into a flat buffer (0x5A-filled first). scale None: the unscaled entry
    (ddl_pack / ddl_pack_cvt / ddl_pack_cvt_fb). Returns (flat bytes, the residuals afterwards)."""
    k, lens = len(xs), [len(x) for x in xs]
    es = 2 if wire else 4
    offs, total = _layout(lens, misaligned)
    host = np.full(total, GUARD, np.uint8)
    for x, o in zip(xs, offs):
        host[o:o + 4 * len(x)] = x.view(np.uint8)
    src = torch.from_numpy(host).to(gpu)
    flat = torch.full((max(256, sum(_round256(n * es) for n in lens)),), 0x5A, dtype=torch.uint8, device=gpu)
    srcs = (ctypes.c_void_p * k)(*[src.data_ptr() + o for o in offs])
    elems = (ctypes.c_size_t * k)(*lens)
    res_t, resp = None, None
    if residuals is not None:
        roffs, rtotal = _layout(lens, misaligned)  # residuals share the tensors' alignment pattern
        rh = np.full(rtotal, GUARD, np.uint8)
        for r, o in zip(residuals, roffs):
            if r is not None:
                rh[o:o + 4 * len(r)] = r.view(np.uint8)
        res_t = torch.from_numpy(rh).to(gpu)
        resp = (ctypes.c_void_p * k)(*[res_t.data_ptr() + o if r is not None else None
                                       for r, o in zip(residuals, roffs)])
    if scale is not None:
        st = lib.ddl_pack_scale(flat.data_ptr(), srcs, resp, elems, k, wire, _floats(k, scale), _stream())
    elif not wire:
        st = lib.ddl_pack(flat.data_ptr(), srcs, (ctypes.c_size_t * k)(*[4 * n for n in lens]), k, _stream())
    elif residuals is None:
        st = lib.ddl_pack_cvt(flat.data_ptr(), srcs, elems, k, wire, _stream())
    else:
        st = lib.ddl_pack_cvt_fb(flat.data_ptr(), srcs, resp, elems, k, wire, _stream())
    assert st == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    assert src.cpu().numpy().tobytes() == host.tobytes(), 'a pack wrote to its sources'
    out_res = None
    if residuals is not None:
        got = res_t.cpu().numpy()
        covered = np.zeros(got.size, bool)
        for r, o in zip(residuals, roffs):
            if r is not None:
                covered[o:o + 4 * len(r)] = True
        assert (got[~covered] == GUARD).all(), 'bytes outside the residuals were written'
        out_res = [got[o:o + 4 * len(r)].view(np.float32).copy() if r is not None else None
                   for r, o in zip(residuals, roffs)]
    return flat.cpu().numpy(), out_res


def _unpack(lib, gpu, data, wire, ops, scale=None, want=None, misaligned=(), in_place=False):
    """Scatter the flat side's contents `data` (fp32 values, or wire bit patterns) into guarded tensors.
    scale None: the unscaled entries. Returns (destination bytes, offsets, sums of squares or None)."""
    k, lens = len(data), [len(x) for x in data]
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
    cops = (ctypes.c_int * k)(*ops)
    sp = None if in_place else src.data_ptr()
    out = (ctypes.c_double * k)(*([-1.0] * k))
    cw = (ctypes.c_ubyte * k)(*want) if want is not None else None
    if scale is not None:
        st = lib.ddl_unpack_scale(dsts, sp, (ctypes.c_size_t * k)(*lens), cops, k, wire, P, _floats(k, scale), _stream(),
                                  cw, out if want is not None else None)
    else:
        sizes = (ctypes.c_size_t * k)(*[n if wire else 4 * n for n in lens])
        if want is None:
            fn = lib.ddl_unpack_cvt if wire else lib.ddl_unpack_ops
            st = fn(dsts, sp, sizes, cops, k, wire if wire else DT_FLOAT, P, _stream())
        else:
            fn = lib.ddl_unpack_cvt_sumsq if wire else lib.ddl_unpack_ops_sumsq
            st = fn(dsts, sp, sizes, cops, k, wire if wire else DT_FLOAT, P, _stream(), cw, out)
    assert st == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    covered = np.zeros(got.size, bool)
    for o, n in zip(offs, lens):
        covered[o:o + 4 * n] = True
    assert (got[~covered] == GUARD).all(), 'bytes outside the segments were written'
    return got, offs, (list(out) if want is not None else None)


def _segments(got, offs, lens):
    return [got[o:o + 4 * n].view(np.float32) for o, n in zip(offs, lens)]


def _same_double(a, b):
    return (math.isnan(a) and math.isnan(b)) or struct.pack('<d', a) == struct.pack('<d', b)


def _inputs(factors, seed, lens=LENS):
    return [scale_input(n, seed + i, f) for i, (n, f) in enumerate(zip(lens, factors))]


def _wire_data(xs, wire):
    """What the flat buffer of an unpack holds: fp32 values, or their wire roundings' bit patterns."""
    if not wire:
        return xs
    return [narrow(wire, x).view(np.uint16) for x in xs]


@_cases(WIRES, WIRE_IDS)
def test_scaled_packs(lib, gpu, wire, geo):
    """Every scaled pack's flat buffer is the unscaled pack's of NumPy-premultiplied inputs — the 0x5A
    padding between the segments included — and a factor-1 segment in the launch has the plain bytes."""
    lens, misaligned, fshift, _ = GEOMETRIES[geo]
    for shift in (0, 1, 3):
        fs = mixed_factors(len(lens), shift + fshift)
        assert any(f == 1 and n for f, n in zip(fs, lens)) and any(f != 1 and n for f, n in zip(fs, lens))
        xs = _inputs(fs, 100 * shift, lens)
        got, _ = _pack(lib, gpu, xs, wire, fs, misaligned=misaligned)
        ref, _ = _pack(lib, gpu, [mul(x, f) for x, f in zip(xs, fs)], wire, None, misaligned=misaligned)
        assert same_bits(_flat_values(got, wire), _flat_values(ref, wire)), (wire, shift)
        plain, _ = _pack(lib, gpu, xs, wire, None, misaligned=misaligned)
        off, es = 0, 2 if wire else 4
        for x, f in zip(xs, fs):
            if f == 1:
                assert got[off:off + es * len(x)].tobytes() == plain[off:off + es * len(x)].tobytes()
            pad = slice(off + es * len(x), off + _round256(es * len(x)))
            assert (got[pad] == 0x5A).all(), 'padding between segments was written'
            off += _round256(es * len(x))


def test_all_factors_one_is_the_plain_launch(lib, gpu):
    xs = _inputs([1.0] * len(LENS), 7)
    for wire in WIRES:
        got, _ = _pack(lib, gpu, xs, wire, [1.0] * len(LENS), misaligned=MISALIGNED)
        ref, _ = _pack(lib, gpu, xs, wire, None, misaligned=MISALIGNED)
        assert got.tobytes() == ref.tobytes()
        data = _wire_data(xs, wire)
        ops = [OP_AVG if i % 2 else OP_SUM for i in range(len(LENS))]
        got, _, _ = _unpack(lib, gpu, data, wire, ops, [1.0] * len(LENS), misaligned=MISALIGNED)
        ref, _, _ = _unpack(lib, gpu, data, wire, ops, None, misaligned=MISALIGNED)
        assert got.tobytes() == ref.tobytes()


@_cases([DT_HALF, DT_BFLOAT16], ['fp16', 'bf16'])
def test_feedback_three_steps(lib, gpu, wire, geo):
    """Three consecutive steps of the scaled feedback pack: wire values and residual bits are the model's;
    segments without a residual and segments without a factor ride in the same launches."""
    lens, misaligned, fshift, no_res = GEOMETRIES[geo]
    fs = mixed_factors(len(lens), 2 + fshift)
    fs[0] = np.float32(1)  # (a second factor-1 segment, this one with a residual)
    has_res = [i not in no_res for i in range(len(lens))]
    assert {(f == 1, h) for f, h, n in zip(fs, has_res, lens) if n} == {(True, True), (True, False), (False, True),
                                                                         (False, False)}
    res = [np.zeros(n, np.float32) if h else None for n, h in zip(lens, has_res)]
    model = [None if r is None else r.copy() for r in res]
    for stepno in range(3):
        xs = _inputs(fs, 1000 + 50 * stepno, lens)
        got, res = _pack(lib, gpu, xs, wire, fs, residuals=res, misaligned=misaligned)
        off = 0
        for i, (x, f) in enumerate(zip(xs, fs)):
            if model[i] is None:
                w = narrow(wire, mul(x, f))
            else:
                w, model[i] = pack_feedback(wire, x, model[i], f)
                assert same_bits(res[i], model[i]), (stepno, i, 'residual')
            have = got[off:off + 2 * len(x)].view(np.float16 if wire == DT_HALF else np.uint16)
            assert same_bits(widen(wire, have), widen(wire, w)), (stepno, i, 'wire')
            off += _round256(2 * len(x))
    assert any(m is not None and np.any(m != 0) for m in model)


@_cases(WIRES, WIRE_IDS)
def test_scaled_unpacks_and_sumsq(lib, gpu, wire, geo):
    """SUM and AVG segments at P = 3 with mixed factors: the scaled unpack stores NumPy's product of the
    unscaled unpack's output; the sumsq form stores the same bytes and its doubles are mirror(out)."""
    lens, misaligned, fshift, _ = GEOMETRIES[geo]
    for shift in (0, 2):
        fs = mixed_factors(len(lens), shift + fshift)
        ops = [OP_AVG if (i + shift) % 2 else OP_SUM for i in range(len(lens))]
        data = _wire_data(_inputs(fs, 300 + shift, lens), wire)
        ref, offs, _ = _unpack(lib, gpu, data, wire, ops, None, misaligned=misaligned)
        got, offs2, _ = _unpack(lib, gpu, data, wire, ops, fs, misaligned=misaligned)
        assert offs == offs2
        for i, (r, g, f) in enumerate(zip(_segments(ref, offs, lens), _segments(got, offs, lens), fs)):
            assert same_bits(g, mul(r, f)), (wire, shift, i)
            if f == 1:
                assert g.tobytes() == r.tobytes(), 'a factor-1 segment differs from the plain kernel'
        want = [0 if i % 3 == 2 else 1 for i in range(len(lens))]
        got2, _, sq = _unpack(lib, gpu, data, wire, ops, fs, want=want, misaligned=misaligned)
        for i, seg in enumerate(_segments(got2, offs, lens)):
            assert same_bits(seg, _segments(got, offs, lens)[i])
            m = mirror(seg, bool(wire)) if want[i] else 0.0
            assert _same_double(sq[i], m), (wire, shift, i, sq[i], m)
        # finite data: the doubles are finite and compared as bits
        clean = _wire_data([np.random.default_rng(i).standard_normal(n).astype(np.float32) for i, n in enumerate(lens)], wire)
        out, _, sq = _unpack(lib, gpu, clean, wire, ops, fs, want=[1] * len(lens), misaligned=misaligned)
        for i, seg in enumerate(_segments(out, offs, lens)):
            m = mirror(seg, bool(wire))
            assert math.isfinite(m) and struct.pack('<d', sq[i]) == struct.pack('<d', m), (i, sq[i], m)


def test_in_place_form(lib, gpu):
    """src == NULL: AVG and scaled segments are rewritten where they are (quotient, then factor, in ONE
    launch), a SUM segment with factor 1 is untouched."""
    fs = mixed_factors(len(LENS), 0)
    ops = [OP_AVG if i % 2 else OP_SUM for i in range(len(LENS))]
    assert any(o == OP_SUM and f == 1 and n for o, f, n in zip(ops, fs, LENS))
    xs = _inputs(fs, 55)
    ref, offs, _ = _unpack(lib, gpu, xs, 0, ops, None, misaligned=MISALIGNED, in_place=True)
    got, _, _ = _unpack(lib, gpu, xs, 0, ops, fs, misaligned=MISALIGNED, in_place=True)
    flat, _, _ = _unpack(lib, gpu, xs, 0, ops, fs, misaligned=MISALIGNED)
    for i, (x, r, g, h, f) in enumerate(zip(xs, _segments(ref, offs, LENS), _segments(got, offs, LENS),
                                            _segments(flat, offs, LENS), fs)):
        assert same_bits(g, mul(r, f)), i
        assert same_bits(g, h), 'in place differs from the scatter'
        if f == 1 and ops[i] == OP_SUM:
            assert g.tobytes() == x.tobytes()


@pytest.mark.parametrize('wire', [DT_HALF, DT_BFLOAT16], ids=['fp16', 'bf16'])
def test_every_16_bit_pattern(lib, gpu, wire):
    """All 65 536 patterns through the scaled converting unpack with b = 1/3 (SUM and AVG at P = 3), and
    all 65 536 values widened to fp32 through the scaled converting pack with a = 1/3."""
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    data, ops = [bits, bits, bits], [OP_SUM, OP_AVG, OP_SUM]
    fs = [THIRD, THIRD, np.float32(1)]
    ref, offs, _ = _unpack(lib, gpu, data, wire, ops, None)
    got, _, sq = _unpack(lib, gpu, data, wire, ops, fs, want=[1, 1, 1])
    lens = [65536] * 3
    vals = widen(wire, bits.view(np.float16) if wire == DT_HALF else bits)
    for i, (r, g) in enumerate(zip(_segments(ref, offs, lens), _segments(got, offs, lens))):
        assert same_bits(g, mul(r, fs[i])), i
        assert math.isnan(sq[i])
    assert same_bits(_segments(got, offs, lens)[0], mul(vals, THIRD))
    fin = bits[np.isfinite(vals)]
    out, o2, sq = _unpack(lib, gpu, [fin, fin], wire, [OP_SUM, OP_AVG], [THIRD, THIRD], want=[1, 1])
    for i, seg in enumerate(_segments(out, o2, [fin.size] * 2)):
        m = mirror(seg, True)
        assert math.isfinite(m) and m > 0 and struct.pack('<d', sq[i]) == struct.pack('<d', m)
    xs = [vals.copy(), vals.copy()]
    got, _ = _pack(lib, gpu, xs, wire, [THIRD, np.float32(1)], misaligned={1})
    ref, _ = _pack(lib, gpu, [mul(vals, THIRD), vals], wire, None, misaligned={1})
    assert same_bits(_flat_values(got, wire), _flat_values(ref, wire))
    model = narrow(wire, mul(vals, THIRD))
    have = got[:2 * 65536].view(np.float16 if wire == DT_HALF else np.uint16)
    assert same_bits(widen(wire, have), widen(wire, model))


def test_bad_factors_are_refused(lib, gpu):
    x = [np.ones(8, np.float32)]
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        k = 1
        t = torch.zeros(64, device=gpu)
        flat = torch.zeros(256, device=gpu)
        srcs = (ctypes.c_void_p * k)(t.data_ptr())
        st = lib.ddl_pack_scale(flat.data_ptr(), srcs, None, (ctypes.c_size_t * k)(8), k, 0, _floats(k, [bad]), _stream())
        assert st == 3, (bad, st)
    got, _ = _pack(lib, gpu, x, 0, [FACTORS[1]])
    assert got[:32].view(np.float32).tolist() == [0.5] * 8
