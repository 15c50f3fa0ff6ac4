"""k_seg<Q8Pack16Op> / k_seg<Q8Unpack16Op> (csrc/pack.hip) through ddl_pack_e4m3_16 / ddl_unpack_e4m3_16, bit for bit
against _e4m3_bf16_helpers.py."""
import ctypes

import numpy as np
import pytest
import torch

import _e4m3_bf16_helpers as h
import _e4m3_helpers as q8
from _bf16_native_helpers import ALL_BITS, assert_same, same_double
from test_e4m3_kernel_gpu import GUARD, _assert_granules, _floats, _stream

pytestmark = pytest.mark.gpu
VP, SZ = ctypes.c_void_p, ctypes.c_size_t
THIRD = float(np.float32(1) / np.float32(3))
# one element, a granule and one past it, a 1 KiB wire tile (4 granules) and one past it, several tiles and a tail
LENS = [1, 252, 253, 1008, 1009, 4 * 1008 + 5]
BASES = [0, 8, 2]  # tensor bases mod 16: both granule parities; 2: below 8 bytes, element by element


def _tensors(lens, base, fill=None):
    """One guarded device allocation holding a bf16 segment per length at `base` mod 16, 48 guard bytes behind each."""
    offs, cur = [], 64
    for n in lens:
        offs.append(((cur + 15) & ~15) + base)
        cur = offs[-1] + 2 * n + 48
    host = np.full(cur + 64, GUARD, np.uint8)
    for x, o in zip(fill or [], offs):
        host[o:o + x.nbytes] = x.view(np.uint8)
    dev = torch.from_numpy(host).cuda()
    return host, dev, offs, (VP * len(lens))(*[dev.data_ptr() + o for o in offs]), (SZ * len(lens))(*lens)


@pytest.mark.parametrize('scaled', [False, True], ids=['plain', 'prescale'])
@pytest.mark.parametrize('base', BASES)
def test_pack_is_the_model(lib, gpu, base, scaled):
    """Every length of LENS and all 65 536 bf16 patterns (in bit order: neighbouring magnitudes share a granule) in one
    launch; `scaled`: a prescale of 1/3 on every other segment, none on the rest."""
    data = [h.rank_input(n, 40 + i) for i, n in enumerate(LENS)] + [ALL_BITS]
    k = len(data)
    scale = [1.0 if i % 2 else THIRD for i in range(k)] if scaled else [1.0] * k
    host, src, _, ptrs, lens = _tensors([x.size for x in data], base, data)
    foffs, ftotal = q8.flat_layout([x.size for x in data])
    flat = torch.full((ftotal + 512,), GUARD, dtype=torch.uint8, device=gpu)
    st = lib.ddl_pack_e4m3_16(flat.data_ptr() + 256, ptrs, lens, k, h.DT_BFLOAT16, _floats(scale) if scaled else None, _stream())
    assert st == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    got = flat.cpu().numpy()
    assert (got[:256] == GUARD).all() and (got[256 + ftotal:] == GUARD).all(), 'the pack wrote outside the flat buffer'
    assert src.cpu().numpy().tobytes() == host.tobytes(), 'the pack wrote to its source'
    for i, (x, o) in enumerate(zip(data, foffs)):
        want = h.pack(x, scale[i])
        _assert_granules(got[256 + o:256 + o + want.size], want, f'segment {i} ({x.size} elements)')


def _granules(codes, scale):
    w = np.zeros((len(codes), 256), np.uint8)
    w[:, :252] = codes
    w[:, 252:] = np.array([scale], np.float32).view(np.uint8)
    return w.ravel()


@pytest.mark.parametrize('base', BASES)
def test_unpack_is_the_model(lib, gpu, base):
    """SUM and AVG (P = 3) segments, a postscale of 1/3 on some, in one launch: every length of LENS, every code under
    the scales 2**-126, 1 and 2**120, and +-1.875 * 2**127 times 1.065, finite in fp32, which overflows only in the
    narrowing. Only the requests' elements are written; the statistic is of the stored bf16 values (2-byte order)."""
    P = 3
    wires = [h.pack(h.rank_input(n, 90 + i, specials=i % 3 == 0)) for i, n in enumerate(LENS)]
    wires += [_granules([np.arange(252), np.arange(4, 256)], s) for s in (2.0 ** -126, 1.0, 2.0 ** 120)]
    wires.append(_granules([[0x77, 0xf7] + [0] * 250], 2.0 ** 120))
    lens = LENS + [504, 504, 504, 2]
    k = len(lens)
    ops = [q8.OP_AVG if i % 2 else q8.OP_SUM for i in range(k - 1)] + [q8.OP_SUM]
    scale = [THIRD if i % 4 >= 2 else 1.0 for i in range(k - 1)] + [1.065]
    fhost = np.concatenate(wires)  # whole granules: the flat layout is their concatenation
    flat = torch.from_numpy(fhost).to(gpu)
    host, dst, toffs, ptrs, nl = _tensors(lens, base)
    sums = (ctypes.c_double * k)()
    st = lib.ddl_unpack_e4m3_16(ptrs, flat.data_ptr(), nl, (ctypes.c_int * k)(*ops), k, h.DT_BFLOAT16, P, _floats(scale),
                                _stream(), (ctypes.c_ubyte * k)(*([1] * k)), sums)
    assert st == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    for i, (w, o) in enumerate(zip(wires, toffs)):
        want = h.unpack(w, lens[i], ops[i], P, scale[i])
        assert_same(got[o:o + want.nbytes].view(np.uint16), want, f'segment {i} ({lens[i]} elements)')
        assert same_double(sums[i], h.sumsq(want)), f'sum of squares of segment {i}'
        host[o:o + want.nbytes] = got[o:o + want.nbytes]
    assert want.tolist() == [0x7f80, 0xff80]  # the last segment: +-inf
    assert got.tobytes() == host.tobytes(), 'bytes outside the segments were written'
    assert flat.cpu().numpy().tobytes() == fhost.tobytes()
