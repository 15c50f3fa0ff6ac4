"""The kernels of the e4m3 wire on their own (csrc/pack.hip k_seg<Q8PackOp> / k_seg<Q8UnpackOp>,
csrc/reduce_kernels.hip k_foldq) through ddl_pack_e4m3 / ddl_unpack_e4m3 / ddl_fold_e4m3, bit for bit against the
CPU model of _e4m3_helpers.py."""
import ctypes

import numpy as np
import pytest
import torch

import _e4m3_helpers as q8
from _avg_helpers import assert_same
from _helpers import DT_FLOAT
from _sumsq_helpers import mirror

pytestmark = pytest.mark.gpu
GUARD = 0xA5
VP, SZ = ctypes.c_void_p, ctypes.c_size_t
# empty, one element, one short of / exactly / one past a granule, the same around a 1 KiB tile (4 granules, 1008
# elements), several tiles and a tail
LENS = [0, 1, 251, 252, 253, 1007, 1008, 1009, 4 * 1008 + 5]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _tensor_layout(lens, misaligned):
    """Byte offsets of the fp32 segments inside one guarded allocation: 16-byte aligned, or one element past it."""
    offs, cur = [], 64
    for n in lens:
        cur = (cur + 15) & ~15
        if misaligned:
            cur += 4
        offs.append(cur)
        cur += 4 * n + (48 if n else 0)  # guard bytes after every non-empty segment
    return offs, cur + 64


def _floats(vals):
    return (ctypes.c_float * len(vals))(*vals)


def _pack(lib, gpu, data, misaligned, scale=None):
    lens = [x.size for x in data]
    toffs, ttotal = _tensor_layout(lens, misaligned)
    host = np.full(ttotal, GUARD, np.uint8)
    for x, o in zip(data, toffs):
        host[o:o + x.nbytes] = x.view(np.uint8)
    src = torch.from_numpy(host).to(gpu)
    foffs, ftotal = q8.flat_layout(lens)
    flat = torch.full((ftotal + 512,), GUARD, dtype=torch.uint8, device=gpu)  # 256 guard bytes on either side
    k = len(lens)
    st = lib.ddl_pack_e4m3(flat.data_ptr() + 256, (VP * k)(*[src.data_ptr() + o for o in toffs]), (SZ * k)(*lens), k,
                           _floats(scale) if scale else None, _stream())
    assert st == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    got = flat.cpu().numpy()
    assert (got[:256] == GUARD).all() and (got[256 + ftotal:] == GUARD).all(), 'the pack wrote outside the flat buffer'
    assert src.cpu().numpy().tobytes() == host.tobytes(), 'the pack wrote to its source'
    return got[256:256 + ftotal], foffs


def _assert_granules(got, want, what):
    assert got.size == want.size, what
    bad = np.flatnonzero(got != want)
    if bad.size:
        b = int(bad[0])
        raise AssertionError(f'{what}: {bad.size} bytes differ, first at granule {b // 256} byte {b % 256}: '
                             f'{got[b]:#x} != {want[b]:#x}')


@pytest.mark.parametrize('scaled', [False, True], ids=['plain', 'prescale'])
@pytest.mark.parametrize('misaligned', [False, True], ids=['aligned16', 'aligned4'])
def test_pack_is_the_model(lib, gpu, misaligned, scaled):
    """Every segment length of LENS in one launch, tensors 16-byte or only 4-byte aligned, guard bytes around the flat
    buffer and the tensors; with `scaled` a prescale of 1/3 on every other segment (1.0: not multiplied)."""
    data = [q8.rank_input(n, 40 + i) for i, n in enumerate(LENS)]
    third = float(np.float32(1) / np.float32(3))
    scale = [third if i % 2 else 1.0 for i in range(len(LENS))] if scaled else None
    got, foffs = _pack(lib, gpu, data, misaligned, scale)
    for i, (x, o) in enumerate(zip(data, foffs)):
        want = q8.pack(x, scale[i] if scaled else 1.0)
        _assert_granules(got[o:o + want.size], want, f'segment {i} ({LENS[i]} elements)')


def _sweep_values(s):
    """For every pair of adjacent e4m3 codes: the midpoint and its two fp32 neighbours, both signs, times the scale s
    (exact), 251 to a granule behind an anchor 448 * s that pins the granule's scale; then NaN, +-inf and -0."""
    d = q8.DECODE[:0x7f].astype(np.float64)
    mid = ((d[:-1] + d[1:]) / 2).astype(np.float32)  # exact: one more bit than a code
    v = (mid.astype(np.float64) * float(s)).astype(np.float32)
    assert np.array_equal(v.astype(np.float64), mid.astype(np.float64) * float(s))
    vals = np.concatenate([np.nextafter(v, np.float32(0)), v, np.nextafter(v, np.float32(np.inf))])
    neg_nan = np.array([0xffc00000], np.uint32).view(np.float32)
    vals = np.concatenate([vals, -vals, np.array([np.nan, np.inf, -np.inf, -0.0], np.float32), neg_nan])
    vals = vals[np.abs(np.nan_to_num(vals, posinf=0, neginf=0)) <= np.float32(448.0) * s]  # (the neighbour above 448 s)
    out = []
    for i in range(0, vals.size, 251):
        out.append(np.float32(448.0) * s)
        out.extend(vals[i:i + 251])
    return np.array(out, np.float32)


@pytest.mark.parametrize('exp', [-126, 0, 100])
def test_rounding_sweep(lib, gpu, exp):
    """Round to nearest even with subnormal codes and -0 kept, over every tie of the format and its fp32 neighbours,
    in granules whose scale is 2**exp."""
    s = np.ldexp(np.float32(1), exp)
    x = _sweep_values(s)
    got, _ = _pack(lib, gpu, [x], False)
    want = q8.pack(x)
    assert (want.reshape(-1, 256)[:, 252:].copy().view(np.float32) == s).all()
    _assert_granules(got, want, f'scale 2**{exp}')


def _crafted_inputs(nin, ng, seed):
    """nin inputs of ng granules: packed gradients (specials in input 0 only), then crafted granules: all-zero bytes
    (a scale of 0), all-zero codes, the largest scale with the largest codes (the sum overflows), the smallest scale,
    NaN codes of either sign (one input per position) and a NaN scale."""
    ins = [q8.pack(q8.rank_input(ng * q8.G - 7, seed, r)).reshape(ng, 256).copy() for r in range(nin)]
    def bits(u):
        return np.array([u], np.uint32).view(np.uint8)
    for r, w in enumerate(ins):
        w[3] = 0  # zero bytes everywhere, the scale included
        w[4, :252] = 0
        w[5, :252] = 0x7e if r % 2 == 0 else 0x7d
        w[5, 252:] = bits(247 << 23)  # 2**120
        w[6, 252:] = bits(1 << 23)  # 2**-126: the products are fp32 subnormals
        w[7, :252] &= 0x7e  # no NaN codes from the specials in this one
    ins[0][7, 10] = 0x7f
    ins[min(1, nin - 1)][7, 20] = 0xff
    ins[nin - 1][8, 252:] = bits(0x7fc00000)
    return [w.ravel() for w in ins]


@pytest.mark.parametrize('nb', [1, 2, 7, 15])
def test_fold_is_the_model(lib, gpu, nb):
    """nb + 1 inputs over 29 granules (three whole 2 KiB tiles and a partial one), guard bytes behind the output."""
    ng = 29
    ins = _crafted_inputs(nb + 1, ng, 70 + nb)
    dev = [torch.from_numpy(w).to(gpu) for w in ins]
    out = torch.full((ng * 256 + 256,), GUARD, dtype=torch.uint8, device=gpu)
    st = lib.ddl_fold_e4m3(out.data_ptr(), dev[0].data_ptr(), (VP * nb)(*[t.data_ptr() for t in dev[1:]]), nb, ng,
                           _stream())
    assert st == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[ng * 256:] == GUARD).all(), 'the fold wrote past its output'
    for t, w in zip(dev, ins):
        assert t.cpu().numpy().tobytes() == w.tobytes(), 'the fold wrote to an input'
    _assert_granules(got[:ng * 256], q8.fold(ins), f'{nb + 1} inputs')


@pytest.mark.parametrize('misaligned', [False, True], ids=['aligned16', 'aligned4'])
def test_unpack_is_the_model(lib, gpu, misaligned):
    """SUM and AVG (P = 3) segments, a postscale of 1/3 on some, in one launch; only the requests' elements are
    written; the statistic is the canonical uncompressed sum over what was stored."""
    P, third = 3, float(np.float32(1) / np.float32(3))
    k = len(LENS)
    wires = [q8.pack(q8.rank_input(n, 90 + i, specials=i % 3 == 0)) for i, n in enumerate(LENS)]
    ops = [q8.OP_AVG if i % 2 else q8.OP_SUM for i in range(k)]
    scale = [third if i % 4 >= 2 else 1.0 for i in range(k)]
    want_stat = [1 if i % 3 else 0 for i in range(k)]  # the segments without NaNs
    foffs, ftotal = q8.flat_layout(LENS)
    fhost = np.full(ftotal, 0x5A, np.uint8)
    for w, o in zip(wires, foffs):
        fhost[o:o + w.size] = w
    flat = torch.from_numpy(fhost).to(gpu)
    toffs, ttotal = _tensor_layout(LENS, misaligned)
    dst = torch.full((ttotal,), GUARD, dtype=torch.uint8, device=gpu)
    sums = (ctypes.c_double * k)()
    st = lib.ddl_unpack_e4m3((VP * k)(*[dst.data_ptr() + o for o in toffs]), flat.data_ptr(), (SZ * k)(*LENS),
                             (ctypes.c_int * k)(*ops), k, P, _floats(scale), _stream(),
                             (ctypes.c_ubyte * k)(*want_stat), sums)
    assert st == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    covered = np.zeros(ttotal, bool)
    for i, (w, o) in enumerate(zip(wires, toffs)):
        want = q8.unpack(w, LENS[i], ops[i], P, scale[i])
        covered[o:o + want.nbytes] = True
        assert_same(DT_FLOAT, got[o:o + want.nbytes].view(np.float32), want, f'segment {i} ({LENS[i]} elements)')
        stat = mirror(want, compressed=False) if want_stat[i] else 0.0
        assert np.float64(sums[i]).tobytes() == np.float64(stat).tobytes(), f'sum of squares of segment {i}'
    assert (got[~covered] == GUARD).all(), 'bytes outside the segments were written'
    assert flat.cpu().numpy().tobytes() == fhost.tobytes()


def test_no_statistic_and_bad_arguments(lib, gpu):
    """want NULL is the plain unpack; a null flat buffer and a MIN op are refused."""
    x = q8.rank_input(500, 5, specials=False)
    w = q8.pack(x)
    flat = torch.from_numpy(w).to(gpu)
    dst = torch.zeros(500, dtype=torch.float32, device=gpu)
    one, n1 = (VP * 1)(dst.data_ptr()), (SZ * 1)(500)
    assert lib.ddl_unpack_e4m3(one, flat.data_ptr(), n1, None, 1, 1, None, _stream(), None, None) == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    assert_same(DT_FLOAT, dst.cpu().numpy(), q8.unpack(w, 500), 'plain unpack')
    assert lib.ddl_unpack_e4m3(one, None, n1, None, 1, 1, None, _stream(), None, None) == 3
    assert lib.ddl_unpack_e4m3(one, flat.data_ptr(), n1, (ctypes.c_int * 1)(3), 1, 1, None, _stream(), None, None) == 3
