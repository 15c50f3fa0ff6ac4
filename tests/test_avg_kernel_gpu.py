"""The dividing unpack kernel (csrc/pack.hip k_seg<DivOp>) on its own, through ddl_unpack_ops: the
quotient of DDL_ALLREDUCE_OP_AVG in the store of the fusion scatter, flat -> tensors and in place.

Expected values are the inputs divided on the CPU (numpy; torch CPU for bf16, _avg_helpers.quotient):
fp32 / fp64 the correctly rounded IEEE quotient, fp16 / bf16 through fp32 with one rounding to
nearest even. Everything is compared bit for bit (a NaN must stay a NaN)."""
import ctypes

import numpy as np
import pytest
import torch

from _avg_helpers import FLOAT_DTYPES, OP_AVG, OP_SUM, assert_same, quotient, to_dev, to_host
from _helpers import DT_BFLOAT16, DT_DOUBLE, DT_FLOAT, DT_HALF, NAME, NP, random_input

pytestmark = pytest.mark.gpu
GUARD = 0xA5


def _round256(b):
    return (b + 255) & ~255


def _unpack_ops(lib, dsts, src, nbytes, ops, dt, divisor):
    k = len(dsts)
    st = lib.ddl_unpack_ops((ctypes.c_void_p * k)(*dsts), src, (ctypes.c_size_t * k)(*nbytes),
                            (ctypes.c_int * k)(*ops), k, dt, divisor, torch.cuda.current_stream().cuda_stream)
    assert st == 0, lib.ddl_last_error()
    torch.cuda.synchronize()


def _one_segment(lib, gpu, dt, x, P, in_place=False):
    """x as one AVG segment: the kernel's quotients."""
    src = to_dev(x, gpu)
    dst = src if in_place else torch.zeros_like(src)
    _unpack_ops(lib, [dst.data_ptr()], None if in_place else src.data_ptr(), [x.nbytes], [OP_AVG], dt, P)
    return to_host(dst, dt)


@pytest.mark.parametrize('dt', [DT_HALF, DT_BFLOAT16], ids=lambda d: NAME[d])
def test_every_16_bit_pattern(lib, gpu, dt):
    """All 65536 bit patterns of fp16 / bf16 as one segment, for every tested divisor."""
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    x = bits.view(NP[dt])
    for P in (2, 3, 5, 6, 7, 8, 17, 520):
        assert_same(dt, _one_segment(lib, gpu, dt, x, P), quotient(dt, x, P), f'{NAME[dt]} P={P}')


def _edge_set(dt):
    f = np.finfo(NP[dt])
    tiny, sub = f.tiny, f.smallest_subnormal
    big_sub = np.nextafter(f.tiny, NP[dt](0))  # the largest subnormal
    vals = [0.0, -0.0, sub, -sub, big_sub, -big_sub, tiny, -tiny, f.max, -f.max, np.inf, -np.inf, np.nan,
            # quotients that are subnormal, and that round to or underflow to zero
            tiny * 2, tiny * 3, -tiny * 5, tiny * 16, big_sub * 2, sub * 2, sub * 3, sub * 7, -sub * 8, sub * 9,
            sub * 17, sub * 18, -sub * 34, sub * 5, sub * 6, 1.0, -1.0, 3.0, f.max / 2]
    return np.array(vals, dtype=NP[dt])


@pytest.mark.parametrize('dt', [DT_FLOAT, DT_DOUBLE], ids=lambda d: NAME[d])
def test_ieee_quotient_fp32_fp64(lib, gpu, dt):
    """Edge values and 4096 seeded normals: the correctly rounded quotient, not x * (1 / P). At
    least 100 of the normals must tell the two apart at every P (checked on the CPU first), so a
    reciprocal multiply cannot pass."""
    T = NP[dt]
    normals = np.random.default_rng(20260).standard_normal(4096).astype(T)
    x = np.concatenate([_edge_set(dt), normals])
    for P in (3, 5, 6, 7, 17):
        with np.errstate(all='ignore'):
            witnesses = int(np.count_nonzero(normals / T(P) != normals * (T(1) / T(P))))
        assert witnesses >= 100, (NAME[dt], P, witnesses)
        want = quotient(dt, x, P)
        assert_same(dt, _one_segment(lib, gpu, dt, x, P), want, f'{NAME[dt]} P={P}')
        assert_same(dt, _one_segment(lib, gpu, dt, x, P, in_place=True), want, f'{NAME[dt]} P={P} in place')


def _geometry(es):
    """(element counts, misaligned segment indices): every length at which the kernel takes another
    path, a run of 300 empty segments between two non-empty ones (more than 255 segments in one
    index block: the int32 tile index), some tensor pointers one element off 16-byte alignment."""
    v, t = 16 // es, 1024 // es
    lens = [0, 1, 3, 4, 5, v - 1, v, v + 1, t - 1, t, t + 1, 2 * t + 1, 70_001] + [0] * 300 + [9, 2 * t + 3]
    return lens, {lens.index(t), lens.index(t + 1), lens.index(70_001), len(lens) - 1}


def _layout(lens, misaligned, es):
    """Byte offsets of the segments inside one guarded destination allocation."""
    offs, cur = [], 64
    for i, n in enumerate(lens):
        cur = (cur + 15) & ~15
        if i in misaligned:
            cur += es
        offs.append(cur)
        cur += n * es + (48 if n else 0)  # guard bytes after every non-empty segment
    return offs, cur + 64


def _segment_data(dt, lens, seed):
    return [random_input(dt, n, seed + i) for i, n in enumerate(lens)]


@pytest.mark.parametrize('all_avg', [False, True], ids=['alternating', 'all_avg'])
@pytest.mark.parametrize('dt', FLOAT_DTYPES, ids=lambda d: NAME[d])
def test_segment_geometry_flat_to_tensors(lib, gpu, dt, all_avg):
    """Mixed SUM / AVG segments in one launch: AVG segments are the quotients, SUM segments the
    input's bytes, and no byte of the destination outside the segments is written."""
    es, P = np.dtype(NP[dt]).itemsize, 3
    lens, mis = _geometry(es)
    data = _segment_data(dt, lens, 500)
    nonempty = [i for i, n in enumerate(lens) if n]
    # non-empty segments alternate SUM, AVG, ...; the empty ones carry both ops too
    ops = [OP_AVG if all_avg or (nonempty.index(i) if n else i) % 2 == 1 else OP_SUM for i, n in enumerate(lens)]
    flat = np.full(sum(_round256(n * es) for n in lens), 0x5A, np.uint8)
    off = 0
    for x in data:
        flat[off:off + x.nbytes] = x.view(np.uint8)
        off += _round256(x.nbytes)
    offs, total = _layout(lens, mis, es)
    dst = torch.full((total,), GUARD, dtype=torch.uint8, device=gpu)
    src = torch.from_numpy(flat).to(gpu)
    _unpack_ops(lib, [dst.data_ptr() + o for o in offs], src.data_ptr(), [n * es for n in lens], ops, dt, P)
    got = dst.cpu().numpy()
    covered = np.zeros(total, bool)
    for i, (x, o) in enumerate(zip(data, offs)):
        seg = got[o:o + x.nbytes].view(NP[dt])
        covered[o:o + x.nbytes] = True
        if ops[i] == OP_AVG:
            assert_same(dt, seg, quotient(dt, x, P), f'segment {i} ({lens[i]} elements)')
        else:
            assert seg.tobytes() == x.tobytes(), f'SUM segment {i} ({lens[i]} elements) changed'
    assert (got[~covered] == GUARD).all(), 'bytes outside the segments were written'


@pytest.mark.parametrize('dt', FLOAT_DTYPES, ids=lambda d: NAME[d])
def test_segment_geometry_in_place(lib, gpu, dt):
    """Source = destination: AVG segments are divided where they are; SUM segments and every
    other byte of the allocation stay as they were."""
    es, P = np.dtype(NP[dt]).itemsize, 3
    lens, mis = _geometry(es)
    data = _segment_data(dt, lens, 900)
    nonempty = [i for i, n in enumerate(lens) if n]
    ops = [OP_AVG if n and nonempty.index(i) % 2 == 0 else OP_SUM for i, n in enumerate(lens)]
    offs, total = _layout(lens, mis, es)
    before = np.full(total, GUARD, np.uint8)
    for x, o in zip(data, offs):
        before[o:o + x.nbytes] = x.view(np.uint8)
    buf = torch.from_numpy(before).to(gpu)
    _unpack_ops(lib, [buf.data_ptr() + o for o in offs], None, [n * es for n in lens], ops, dt, P)
    got = buf.cpu().numpy()
    want = before.copy()
    for i, (x, o) in enumerate(zip(data, offs)):
        if ops[i] == OP_AVG:
            assert_same(dt, got[o:o + x.nbytes].view(NP[dt]), quotient(dt, x, P), f'segment {i} ({lens[i]} elements)')
            want[o:o + x.nbytes] = got[o:o + x.nbytes]
    assert got.tobytes() == want.tobytes(), 'bytes outside the AVG segments changed'


def test_all_sum_and_divisor_one_are_the_plain_unpack(lib, gpu):
    """No AVG segment, or a divisor of 1: the copy, bit for bit (the plain kernels run)."""
    x = random_input(DT_FLOAT, 5000, 3)
    for ops, P in (([OP_SUM], 3), ([OP_AVG], 1)):
        src, dst = to_dev(x, gpu), torch.zeros(5000, dtype=torch.float32, device=gpu)
        _unpack_ops(lib, [dst.data_ptr()], src.data_ptr(), [x.nbytes], ops, DT_FLOAT, P)
        assert to_host(dst, DT_FLOAT).tobytes() == x.tobytes()
