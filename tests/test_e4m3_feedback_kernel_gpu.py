"""The feedback form of the e4m3 pack on its own (csrc/pack.hip k_seg<Q8PackOp<SCALE, true>>) through
ddl_pack_e4m3_fb, bit for bit — wire and residual — against the CPU model of _e4m3_feedback_helpers.py."""
import ctypes

import numpy as np
import pytest
import torch

import _e4m3_feedback_helpers as fb
import _e4m3_helpers as q8

pytestmark = pytest.mark.gpu
GUARD = 0xA5
VP, SZ = ctypes.c_void_p, ctypes.c_size_t
F = np.float32
THIRD = float(F(1) / F(3))
# one element, one short of / exactly / one past a granule, one past a 1 KiB tile, many tiles and a tail
LENS = [1, 251, 252, 253, 1009, 20_011]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _layout(lens, shift):
    """Byte offsets of fp32 arrays inside one guarded allocation: array i 16-byte aligned plus shift[i] bytes, 48
    guard bytes behind each."""
    offs, cur = [], 64
    for n, sh in zip(lens, shift):
        cur = ((cur + 15) & ~15) + sh
        offs.append(cur)
        cur += 4 * n + 48
    return offs, cur + 64


def _upload(arrays, offs, total, gpu):
    host = np.full(total, GUARD, np.uint8)
    for x, o in zip(arrays, offs):
        host[o:o + x.nbytes] = x.view(np.uint8)
    return host, torch.from_numpy(host).to(gpu)


def _pack_fb(lib, gpu, data, residuals, use, misaligned, scale=None, plain=False):
    """One launch over `data`. residuals[i]: segment i's residual before the launch; use[i]: whether its address is
    handed over (else NULL: the memory must stay as it is). The tensors 16-byte aligned or 4 bytes off; the residuals
    alternate between the two WHATEVER the tensors do (the residual's vector path is its own). plain: ddl_pack_e4m3.
    Returns (the flat buffer's bytes, its segment offsets, the residuals after the launch)."""
    lens = [x.size for x in data]
    k = len(lens)
    toffs, ttotal = _layout(lens, [4 if misaligned else 0] * k)
    roffs, rtotal = _layout(lens, [4 * (i % 2) for i in range(k)])
    thost, src = _upload(data, toffs, ttotal, gpu)
    rhost, res = _upload(residuals, roffs, rtotal, gpu)
    foffs, ftotal = q8.flat_layout(lens)
    flat = torch.full((ftotal + 512,), GUARD, dtype=torch.uint8, device=gpu)  # 256 guard bytes on either side
    S = (VP * k)(*[src.data_ptr() + o for o in toffs])
    sc = (ctypes.c_float * k)(*scale) if scale else None
    if plain:
        st = lib.ddl_pack_e4m3(flat.data_ptr() + 256, S, (SZ * k)(*lens), k, sc, _stream())
    else:
        R = (VP * k)(*[res.data_ptr() + o if u else None for o, u in zip(roffs, use)])
        st = lib.ddl_pack_e4m3_fb(flat.data_ptr() + 256, S, R, (SZ * k)(*lens), k, sc, _stream())
    assert st == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    got = flat.cpu().numpy()
    assert (got[:256] == GUARD).all() and (got[256 + ftotal:] == GUARD).all(), 'the pack wrote outside the flat buffer'
    assert src.cpu().numpy().tobytes() == thost.tobytes(), 'the pack wrote to its source'
    rgot = res.cpu().numpy()
    keep = np.ones(rtotal, bool)  # everything but the n elements of the residuals handed over: guards, NULL segments
    for n, o, u in zip(lens, roffs, use):
        if u:
            keep[o:o + 4 * n] = False
    assert (rgot[keep] == rhost[keep]).all(), 'a byte outside the residuals handed over was written'
    return got[256:256 + ftotal], foffs, [rgot[o:o + 4 * n].copy().view(F) for n, o in zip(lens, roffs)]


def _assert_bytes(got, want, what):
    got, want = np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)
    assert got.size == want.size, what
    bad = np.flatnonzero(got != want)
    if bad.size:
        b = int(bad[0])
        raise AssertionError(f'{what}: {bad.size} bytes differ, first at byte {b} (granule {b // 256} byte {b % 256} / '
                             f'element {b // 4}): {got[b]:#x} != {want[b]:#x}')


@pytest.fixture(scope='module')
def inputs():
    """The tensors (NaN, +-inf, -0.0 and an fp32 subnormal among them) and residuals as a previous step left them."""
    return ([q8.rank_input(n, 60 + i) for i, n in enumerate(LENS)],
            [fb.residual_seed(n, 60 + i) for i, n in enumerate(LENS)])


@pytest.mark.parametrize('every_other', [False, True], ids=['all', 'every_other_null'])
@pytest.mark.parametrize('scaled', [False, True], ids=['plain', 'prescale'])
@pytest.mark.parametrize('misaligned', [False, True], ids=['aligned16', 'aligned4'])
def test_pack_fb_is_the_model(lib, gpu, inputs, misaligned, scaled, every_other):
    """Every segment length of LENS in one launch: wire and residual are the model's, the guard words behind every
    residual's n elements and around the flat buffer are unchanged (checked in _pack_fb). With `every_other` the odd
    segments have no residual: they are what ddl_pack_e4m3 packs and their would-be residual memory is untouched."""
    data, res = inputs
    k = len(LENS)
    scale = [THIRD if i % 3 != 2 else 1.0 for i in range(k)] if scaled else None
    use = [not (every_other and i % 2) for i in range(k)]
    got, foffs, rgot = _pack_fb(lib, gpu, data, res, use, misaligned, scale)
    plain = _pack_fb(lib, gpu, data, res, [False] * k, misaligned, scale, plain=True)[0] if every_other else None
    for i, (x, o) in enumerate(zip(data, foffs)):
        a = scale[i] if scaled else 1.0
        what = f'segment {i} ({LENS[i]} elements)'
        if use[i]:
            want, rwant = fb.pack_fb(x, res[i], a)
            _assert_bytes(rgot[i], rwant, what + ' residual')
        else:
            want = q8.pack(x, a)
            _assert_bytes(got[o:o + want.size], plain[o:o + want.size], what + " against ddl_pack_e4m3's bytes")
        _assert_bytes(got[o:o + want.size], want, what + ' wire')


def test_three_chained_steps(lib, gpu):
    """One residual carried through three launches equals the model's three steps; a NaN or an infinity of the first
    step leaves +0.0 behind and nothing of it in the later ones."""
    k = len(LENS)
    res = [np.zeros(n, F) for n in LENS]
    want_res = [np.zeros(n, F) for n in LENS]
    for step in range(3):
        data = [q8.rank_input(n, 80 + i + 100 * step, specials=step == 0) for i, n in enumerate(LENS)]
        got, foffs, res = _pack_fb(lib, gpu, data, res, [True] * k, step == 1, [THIRD] * k if step == 2 else None)
        for i, (x, o) in enumerate(zip(data, foffs)):
            want, want_res[i] = fb.pack_fb(x, want_res[i], THIRD if step == 2 else 1.0)
            _assert_bytes(got[o:o + want.size], want, f'step {step} segment {i} wire')
            _assert_bytes(res[i], want_res[i], f'step {step} segment {i} residual')
            assert np.isfinite(res[i]).all()


def test_every_residual_null_is_the_plain_pack(lib, gpu, inputs):
    data, res = inputs
    k = len(LENS)
    for misaligned in (False, True):
        got = _pack_fb(lib, gpu, data, res, [False] * k, misaligned)[0]
        _assert_bytes(got, _pack_fb(lib, gpu, data, res, [False] * k, misaligned, plain=True)[0], 'all NULL')
