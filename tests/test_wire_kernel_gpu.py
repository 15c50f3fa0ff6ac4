"""The converting fusion kernels (csrc/pack.hip k_seg<CvtPackOp> / k_seg<CvtUnpackOp>) on their own,
through ddl_pack_cvt / ddl_unpack_cvt, for both wire types.

Expected values are the CPU's casts (_wire_helpers.narrow / widen: numpy for fp16, torch CPU for
bf16) and numpy's fp32 quotient; everything is compared bit for bit (a NaN must stay a NaN)."""
import ctypes

import numpy as np
import pytest
import torch

from _avg_helpers import assert_same
from _helpers import DT_FLOAT, DT_HALF
from _wire_helpers import OP_AVG, OP_SUM, WIRE_NAME, WIRES, narrow, widen, wire_input

pytestmark = pytest.mark.gpu
GUARD = 0xA5
# odd counts, below one 8-element vector, one vector, no tile multiple (a tile is 512 elements),
# one element past a tile, several tiles; 300 and 70_001 on a pointer that is only 4-byte aligned
ELEMENTS = [1, 5, 7, 8, 300, 513, 4099, 70_001]
MISALIGNED = {4, 7}
# more than 255 empty segments inside one 128-tile index block: the int32 tile map
WIDE = [3000, 17] + [0] * 300 + [5, 2048]
GEOMETRIES = {'edges': (ELEMENTS, MISALIGNED), 'wide_map': (WIDE, {1})}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _round256(b):
    return (b + 255) & ~255


def _tensor_layout(lens, misaligned):
    """Byte offsets of the fp32 segments inside one guarded allocation: 16-byte aligned, or one
    element past it."""
    offs, cur = [], 64
    for i, n in enumerate(lens):
        cur = (cur + 15) & ~15
        if i in misaligned:
            cur += 4
        offs.append(cur)
        cur += 4 * n + (48 if n else 0)  # guard bytes after every non-empty segment
    return offs, cur + 64


def _flat_layout(lens):
    offs, cur = [], 0
    for n in lens:
        offs.append(cur)
        cur += _round256(2 * n)
    return offs, cur


@pytest.mark.parametrize('geometry', list(GEOMETRIES))
@pytest.mark.parametrize('wire', WIRES, ids=lambda d: WIRE_NAME[d])
def test_pack_is_the_cpu_cast(lib, gpu, wire, geometry):
    """Every segment of the flat buffer holds the round-to-nearest-even cast of its tensor; the
    padding between the segments is not written."""
    lens, mis = GEOMETRIES[geometry]
    data = [wire_input(n, 4000 + i) for i, n in enumerate(lens)]
    toffs, ttotal = _tensor_layout(lens, mis)
    host = np.full(ttotal, GUARD, np.uint8)
    for x, o in zip(data, toffs):
        host[o:o + x.nbytes] = x.view(np.uint8)
    src = torch.from_numpy(host).to(gpu)
    foffs, ftotal = _flat_layout(lens)
    flat = torch.full((ftotal,), GUARD, dtype=torch.uint8, device=gpu)
    k = len(lens)
    st = lib.ddl_pack_cvt(flat.data_ptr(), (ctypes.c_void_p * k)(*[src.data_ptr() + o for o in toffs]),
                          (ctypes.c_size_t * k)(*lens), k, wire, _stream())
    assert st == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    got = flat.cpu().numpy()
    covered = np.zeros(ftotal, bool)
    for i, (x, o) in enumerate(zip(data, foffs)):
        want = narrow(wire, x)
        covered[o:o + want.nbytes] = True
        assert_same(wire, got[o:o + want.nbytes].view(want.dtype), want, f'segment {i} ({lens[i]} elements)')
    assert (got[~covered] == GUARD).all(), 'padding of the flat buffer was written'
    assert src.cpu().numpy().tobytes() == host.tobytes(), 'the pack wrote to its source'


@pytest.mark.parametrize('geometry', list(GEOMETRIES))
@pytest.mark.parametrize('wire', WIRES, ids=lambda d: WIRE_NAME[d])
def test_unpack_widens_and_divides(lib, gpu, wire, geometry):
    """Divisor 3, SUM and AVG segments in one launch: SUM segments are the widened wire values, AVG
    segments their fp32 quotients by 3.0f, and no byte outside the segments is written."""
    lens, mis = GEOMETRIES[geometry]
    P = 3
    wires = [narrow(wire, wire_input(n, 6000 + i)) for i, n in enumerate(lens)]
    nonempty = [i for i, n in enumerate(lens) if n]
    ops = [OP_AVG if (nonempty.index(i) if n else i) % 2 == 1 else OP_SUM for i, n in enumerate(lens)]
    foffs, ftotal = _flat_layout(lens)
    fhost = np.full(ftotal, 0x5A, np.uint8)
    for w, o in zip(wires, foffs):
        fhost[o:o + w.nbytes] = w.view(np.uint8)
    flat = torch.from_numpy(fhost).to(gpu)
    toffs, ttotal = _tensor_layout(lens, mis)
    dst = torch.full((ttotal,), GUARD, dtype=torch.uint8, device=gpu)
    k = len(lens)
    st = lib.ddl_unpack_cvt((ctypes.c_void_p * k)(*[dst.data_ptr() + o for o in toffs]), flat.data_ptr(),
                            (ctypes.c_size_t * k)(*lens), (ctypes.c_int * k)(*ops), k, wire, P, _stream())
    assert st == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    covered = np.zeros(ttotal, bool)
    for i, (w, o) in enumerate(zip(wires, toffs)):
        want = widen(wire, w)
        if ops[i] == OP_AVG:
            with np.errstate(all='ignore'):
                want = (want / np.float32(P)).astype(np.float32)
        covered[o:o + want.nbytes] = True
        assert_same(DT_FLOAT, got[o:o + want.nbytes].view(np.float32), want,
                    f'segment {i} ({lens[i]} elements, op {ops[i]})')
    assert (got[~covered] == GUARD).all(), 'bytes outside the segments were written'


@pytest.mark.parametrize('wire', WIRES, ids=lambda d: WIRE_NAME[d])
def test_true_division_not_a_reciprocal(lib, gpu, wire):
    """Every finite 16-bit pattern widened and divided by 3, 5, 7: the correctly rounded fp32
    quotient. At least 100 patterns per divisor tell it from x * (1 / P) (checked on the CPU)."""
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    w = bits.view(np.float16) if wire == DT_HALF else bits
    x = widen(wire, w)
    flat = torch.from_numpy(bits.view(np.int16).copy()).to(gpu)
    for P in (3, 5, 7):
        with np.errstate(all='ignore'):
            want = (x / np.float32(P)).astype(np.float32)
            other = x * (np.float32(1) / np.float32(P))
        assert np.count_nonzero(want[np.isfinite(x)] != other[np.isfinite(x)]) >= 100
        dst = torch.zeros(65536, dtype=torch.float32, device=gpu)
        st = lib.ddl_unpack_cvt((ctypes.c_void_p * 1)(dst.data_ptr()), flat.data_ptr(), (ctypes.c_size_t * 1)(65536),
                                (ctypes.c_int * 1)(OP_AVG), 1, wire, P, _stream())
        assert st == 0, lib.ddl_last_error()
        torch.cuda.synchronize()
        assert_same(DT_FLOAT, dst.cpu().numpy(), want, f'{WIRE_NAME[wire]} P={P}')


def test_bad_wire_dtype_is_refused(lib, gpu):
    x = torch.zeros(16, dtype=torch.float32, device=gpu)
    one, n1 = (ctypes.c_void_p * 1)(x.data_ptr()), (ctypes.c_size_t * 1)(8)
    assert lib.ddl_pack_cvt(x.data_ptr(), one, n1, 1, DT_FLOAT, _stream()) == 4  # UNSUPPORTED_DTYPE
    assert lib.ddl_unpack_cvt(one, x.data_ptr(), n1, None, 1, 2, 1, _stream()) == 4
