"""The bf16 converting pack with stochastic rounding (csrc/pack.hip k_seg<CvtPackSrOp>) on its own, through
ddl_pack_cvt_sr with caller-supplied stream keys and first element indices.

Expected values are the NumPy mirror's (_stochastic_helpers.sr: the header's R, rule and nothing else), bit
for bit; the segments without the bit must hold ddl_pack_cvt's bytes. Guard bytes lie before and after the
flat buffer, in its padding and around every tensor; none may change."""
import ctypes

import numpy as np
import pytest
import torch

import _stochastic_helpers as sh
from _avg_helpers import assert_same
from _helpers import DT_BFLOAT16
from _scale_helpers import mul
from _wire_helpers import narrow, wire_input
from test_wire_kernel_gpu import _flat_layout, _tensor_layout

pytestmark = pytest.mark.gpu
GUARD = 0xA5
FLAT_GUARD = 256
# below one 8-element vector, one vector, one past it, around one 512-element tile, 32 tiles and one element,
# more than one 128-tile index block; then more than 255 empty segments inside one index block (the int32
# tile map), then two more segments
LENS = [0, 1, 3, 7, 8, 9, 511, 512, 513, 16385, 70_001] + [0] * 300 + [9, 515]
LIVE = [i for i, n in enumerate(LENS) if n]
MISALIGNED = {5, 8, 10, len(LENS) - 1}  # 9, 513, 70_001 and 515 elements on a pointer that is only 4-byte aligned
FIRSTS = [0, 1, 7, 8, 128, 2 ** 32 + 5]  # even, odd, a vector, a tile cut, past 2^32 at an odd index


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _pack(lib, gpu, lens, data, mis, want, keys, firsts, scale=None, plain=False, residuals=None):
    """One launch; returns the segments' wire values (uint16 arrays) after checking every guard byte."""
    k = len(lens)
    toffs, ttotal = _tensor_layout(lens, mis)
    host = np.full(ttotal, GUARD, np.uint8)
    for x, o in zip(data, toffs):
        host[o:o + x.nbytes] = x.view(np.uint8)
    src = torch.from_numpy(host).to(gpu)
    foffs, ftotal = _flat_layout(lens)
    flat = torch.full((ftotal + 2 * FLAT_GUARD,), GUARD, dtype=torch.uint8, device=gpu)
    assert src.data_ptr() % 16 == 0 and flat.data_ptr() % 256 == 0
    S = (ctypes.c_void_p * k)(*[src.data_ptr() + o for o in toffs])
    N = (ctypes.c_size_t * k)(*lens)
    if plain:
        st = lib.ddl_pack_cvt(flat.data_ptr() + FLAT_GUARD, S, N, k, DT_BFLOAT16, _stream())
    else:
        st = lib.ddl_pack_cvt_sr(flat.data_ptr() + FLAT_GUARD, S, residuals, N, k, (ctypes.c_ubyte * k)(*want),
                                 (ctypes.c_ulonglong * k)(*keys), (ctypes.c_ulonglong * k)(*firsts),
                                 (ctypes.c_float * k)(*scale) if scale is not None else None, _stream())
    assert st == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    got = flat.cpu().numpy()
    assert (got[:FLAT_GUARD] == GUARD).all() and (got[FLAT_GUARD + ftotal:] == GUARD).all(), \
        'guard bytes before / after the flat buffer were written'
    got = got[FLAT_GUARD:FLAT_GUARD + ftotal]
    covered = np.zeros(ftotal, bool)
    out = []
    for n, o in zip(lens, foffs):
        covered[o:o + 2 * n] = True
        out.append(got[o:o + 2 * n].view(np.uint16).copy())
    assert (got[~covered] == GUARD).all(), 'padding of the flat buffer was written'
    assert src.cpu().numpy().tobytes() == host.tobytes(), 'the pack wrote to its source'
    return out


@pytest.fixture(scope='module')
def data():
    """The segments' inputs (SPECIALS in every head), shared and read-only."""
    xs = [wire_input(n, 9100 + i) for i, n in enumerate(LENS)]
    for x in xs:
        x.setflags(write=False)
    return xs


@pytest.fixture(scope='module')
def plain(lib, gpu, data):
    """ddl_pack_cvt's bytes of the same segments: what a segment without the bit must hold."""
    got = _pack(lib, gpu, LENS, data, MISALIGNED, None, None, None, plain=True)
    for i in LIVE:
        assert_same(DT_BFLOAT16, got[i], narrow(DT_BFLOAT16, data[i]), f'plain segment {i}')
    return got


@pytest.mark.parametrize('mix', ['all', 'alternating', 'other_half'])
def test_pack_sr_is_the_mirror(lib, gpu, data, plain, mix):
    """Every stochastic segment is the mirror's at its own stream key and first element index (the list of
    first indices walks over the live segments, so every length class meets an odd and an even start);
    every other segment of the same launch holds ddl_pack_cvt's bytes."""
    k = len(LENS)
    rank = {i: j for j, i in enumerate(LIVE)}
    on = [bool(n) and (mix == 'all' or (rank[i] % 2 == 0) == (mix == 'alternating')) for i, n in enumerate(LENS)]
    shift = {'all': 0, 'alternating': 1, 'other_half': 2}[mix]
    keys = [sh.mix64(1000 + i) for i in range(k)]
    firsts = [FIRSTS[(rank.get(i, 0) + shift) % len(FIRSTS)] for i in range(k)]
    got = _pack(lib, gpu, LENS, data, MISALIGNED, on, keys, firsts)
    assert sum(on) >= 5 and (mix == 'all' or sum(on) < len(LIVE))
    for i in LIVE:
        what = f'segment {i} ({LENS[i]} elements, first {firsts[i]}, stochastic {on[i]})'
        if on[i]:
            assert_same(DT_BFLOAT16, got[i], sh.sr(data[i], keys[i], firsts[i]), what)
            if LENS[i] >= 511:
                assert not np.array_equal(got[i], plain[i]), what + ': nothing was rounded the other way'
        else:
            assert np.array_equal(got[i], plain[i]), what


def test_every_first_index_on_every_path(lib, gpu):
    """One 1029-element tensor (two tiles and a partial vector) at every first index, 16-byte aligned (the
    vector path, 4 or 5 words per lane) and 4-byte aligned (the element path): the same bits as the
    mirror's, and the two paths agree."""
    n = 1029
    x = wire_input(n, 9300)
    lens = [n] * (2 * len(FIRSTS))
    firsts = FIRSTS + FIRSTS
    keys = [sh.STREAMS[3]] * len(lens)
    got = _pack(lib, gpu, lens, [x] * len(lens), set(range(len(FIRSTS), len(lens))), [1] * len(lens), keys, firsts)
    for i, f in enumerate(firsts):
        assert_same(DT_BFLOAT16, got[i], sh.sr(x, keys[i], f), f'first {f}, {"element" if i >= len(FIRSTS) else "vector"} path')
    # a piece that starts inside a tensor reads the tensor's own bits
    whole = sh.sr(np.concatenate([np.zeros(128, np.float32), x]), keys[0], 0)[128:]
    assert_same(DT_BFLOAT16, got[FIRSTS.index(128)], whole, 'the piece against the whole tensor')


def test_no_stochastic_segment_is_the_plain_pack(lib, gpu, data, plain):
    """No segment wanted (or only empty ones): the launch is ddl_pack_cvt's, the whole buffer equal."""
    k = len(LENS)
    for want in ([0] * k, [int(n == 0) for n in LENS]):
        got = _pack(lib, gpu, LENS, data, MISALIGNED, want, [sh.STREAMS[1]] * k, [3] * k)
        for i in range(k):
            assert np.array_equal(got[i], plain[i]), f'segment {i}'


def test_prescale_comes_first(lib, gpu):
    """c = g (x) a, then the rule on c; a segment with factor 1 and a plain segment inside the scaled launch."""
    lens = [513, 9, 70_001, 300]
    mis = {1, 2}
    xs = [wire_input(n, 9400 + i) for i, n in enumerate(lens)]
    scale = [np.float32(1.0 / 3.0), np.float32(1.0), np.float32(3.0), np.float32(0.5)]
    on, keys, firsts = [1, 1, 1, 0], [sh.mix64(77 + i) for i in range(4)], [0, 7, 2 ** 32 + 5, 0]
    got = _pack(lib, gpu, lens, xs, mis, on, keys, firsts, scale=scale)
    for i in range(4):
        c = mul(xs[i], scale[i])
        want = sh.sr(c, keys[i], firsts[i]) if on[i] else narrow(DT_BFLOAT16, c)
        assert_same(DT_BFLOAT16, got[i], want, f'segment {i} (factor {scale[i]}, stochastic {on[i]})')


def test_feedback_segments_in_the_same_launch(lib, gpu):
    """A keyed plan may hold requests with the feedback bit next to stochastic ones: one launch with a
    stochastic, a feedback, a plain and again a stochastic segment (vector and element paths, a residual
    that is only 4-byte aligned), twice on the same residuals. The feedback segments follow
    _feedback_helpers.step, the stochastic ones the mirror, the plain one the cast."""
    from _feedback_helpers import step
    lens, mis = [513, 1029, 300, 70_001, 9], {3, 4}
    kinds = ['sr', 'fb', 'plain', 'sr', 'fb']
    keys, firsts = [sh.mix64(500 + i) for i in range(5)], [1, 0, 0, 128, 0]
    resid = [np.zeros(n, np.float32) if kd == 'fb' else None for n, kd in zip(lens, kinds)]
    rbuf = torch.zeros(sum(lens) + 64, dtype=torch.float32, device=gpu)
    roff = {1: 0, 4: 1029 + 4}  # the second residual at a 4-byte-aligned, not 16-byte-aligned, address
    R = (ctypes.c_void_p * 5)(*[rbuf.data_ptr() + 4 * roff[i] if i in roff else None for i in range(5)])
    assert (rbuf.data_ptr() + 4 * roff[4]) % 16 != 0
    for launch in range(2):
        xs = [wire_input(n, 9500 + 10 * launch + i) for i, n in enumerate(lens)]
        got = _pack(lib, gpu, lens, xs, mis, [int(kd == 'sr') for kd in kinds], keys, firsts, residuals=R)
        host = rbuf.cpu().numpy()
        for i, kd in enumerate(kinds):
            what = f'launch {launch} segment {i} ({kd})'
            if kd == 'fb':
                w, resid[i] = step(DT_BFLOAT16, xs[i], resid[i])
                assert_same(DT_BFLOAT16, got[i], w, what)
                assert host[roff[i]:roff[i] + lens[i]].tobytes() == resid[i].tobytes(), what + ': residual'
            else:
                assert_same(DT_BFLOAT16, got[i], sh.sr_or_cast(xs[i], keys[i] if kd == 'sr' else None, firsts[i]), what)
    assert np.count_nonzero(resid[1]) and not host[1029:1033].any() and not host[1033 + 9:].any()  # nothing else written


def test_every_low_half_pattern(lib, gpu):
    """65536 elements holding every low-half pattern under one exponent: each goes up or stays as its own
    random bits say, and the number that goes up is near the 32768 a uniform r gives (exactly the mirror's)."""
    u = np.uint32(0x3f800000) | np.arange(65536, dtype=np.uint32)
    S = sh.STREAMS[2]
    got = _pack(lib, gpu, [65536], [u.view(np.float32)], set(), [1], [S], [0])[0]
    want = sh.sr(u.view(np.float32), S)
    assert np.array_equal(got, want)
    ups = int((got == 0x3f81).sum())
    assert ups == int((want == 0x3f81).sum()) and abs(ups - 32768) < 5 * np.sqrt(65536 / 6)  # sum of p (1 - p)


def test_edge_patterns(lib, gpu):
    """+-0, subnormals, the largest finite value, +-inf and NaNs, at r as the stream gives it and on both paths."""
    x = np.tile(sh.EDGE_BITS, 5).view(np.float32)  # 80 elements: whole vectors
    y = x[:77]                                      # and a partial last vector, element path
    keys = [sh.STREAMS[0], sh.STREAMS[1]]
    got = _pack(lib, gpu, [80, 77], [x, y], {1}, [1, 1], keys, [0, 1])
    for g, v, S, f in zip(got, (x, y), keys, (0, 1)):
        assert_same(DT_BFLOAT16, g, sh.sr(v, S, f), f'edge patterns, first {f}')
        bits = v.view(np.uint32)
        zero = (bits & 0x7fffffff) == 0
        assert np.array_equal(g[zero], (bits[zero] >> 16).astype(np.uint16))  # +-0 stay +-0
        inf = (bits & 0x7fffffff) == 0x7f800000
        assert np.array_equal(g[inf], (bits[inf] >> 16).astype(np.uint16))


def test_bad_arguments_are_refused(lib, gpu):
    x = torch.zeros(16, dtype=torch.float32, device=gpu)
    one, n1 = (ctypes.c_void_p * 1)(x.data_ptr()), (ctypes.c_size_t * 1)(8)
    w, s = (ctypes.c_ubyte * 1)(1), (ctypes.c_ulonglong * 1)(5)
    assert lib.ddl_pack_cvt_sr(x.data_ptr(), one, None, n1, 1, None, s, s, None, _stream()) == 3  # INVALID_ARGUMENT
    assert lib.ddl_pack_cvt_sr(x.data_ptr(), one, None, n1, 1, w, None, s, None, _stream()) == 3
    odd = (ctypes.c_void_p * 1)(x.data_ptr() + 2)  # a tensor that is not 4-byte aligned
    assert lib.ddl_pack_cvt_sr(x.data_ptr(), odd, None, n1, 1, w, s, s, None, _stream()) == 3
    r = torch.zeros(16, dtype=torch.float32, device=gpu)  # one segment cannot be both kinds
    both = (ctypes.c_void_p * 1)(r.data_ptr())
    assert lib.ddl_pack_cvt_sr(x.data_ptr(), one, both, n1, 1, w, s, s, None, _stream()) == 3
    torch.cuda.synchronize()
