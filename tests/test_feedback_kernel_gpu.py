"""The converting pack with error feedback (csrc/pack.hip k_seg<CvtPackOp<WIRE, true>>) on its own, through
ddl_pack_cvt_fb with caller-owned residuals, for both wire types.

Expected values are the CPU model's (_feedback_helpers.step: v = g + r in fp32, the CPU's cast,
r' = v - widen(w) or 0): the bits of the flat buffer and of every residual after each of two
launches in a row on the same residuals. Guard bytes lie before and after the flat buffer, around
every tensor and around every residual; none may change."""
import ctypes

import numpy as np
import pytest
import torch

from _avg_helpers import assert_same
from _feedback_helpers import step_or_cast
from _helpers import DT_FLOAT, random_input
from _wire_helpers import WIRE_NAME, WIRES, wire_input
from test_wire_kernel_gpu import _flat_layout, _tensor_layout

pytestmark = pytest.mark.gpu
GUARD = 0xA5
FLAT_GUARD = 256  # bytes before and after the flat buffer (it stays 256-byte aligned)
# below one 8-element vector, one vector, one past it, around one 512-element tile, several tiles with a tail
EDGES = [0, 1, 7, 8, 9, 511, 512, 513, 1029]
# name -> (segment lengths, segments WITHOUT a residual, tensors offset by 4 bytes, residuals offset by 4 bytes)
GEOMETRIES = {
    # the tensor offset and the residual offset each alone (3, 5 against 6, 8), on vector and tile edges
    'edges_a': (EDGES, {1, 4, 7}, {3, 5}, {6, 8}),
    # the other assignment, with both offsets together on 513 and a misaligned tensor without a residual on 1029
    'edges_b': (EDGES, {2, 5, 8}, {4, 7, 8}, {1, 3, 7}),
    # more than 255 empty segments inside one 128-tile index block: the int32 tile map
    'wide_map': ([3000, 17] + [0] * 300 + [5, 2048], {302}, {1}, {1}),
    # many tiles, more than one 128-tile index block (70_001 elements = 137 tiles)
    'blocks': ([70_001, 300, 40_000], {1}, {2}, {0}),
}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptrs(base, offs, present):
    return (ctypes.c_void_p * len(offs))(*[base + o if p else None for o, p in zip(offs, present)])


def _guarded(arrays, offs, total):
    host = np.full(total, GUARD, np.uint8)
    for x, o in zip(arrays, offs):
        if x is not None:
            host[o:o + x.nbytes] = x.view(np.uint8)
    return host


def _check_guarded(got, arrays, offs, what):
    """Every array's bytes (bit for bit: no NaN can be in a residual) and every guard byte."""
    covered = np.zeros(got.size, bool)
    for i, (x, o) in enumerate(zip(arrays, offs)):
        if x is None:
            continue
        covered[o:o + x.nbytes] = True
        assert_same(DT_FLOAT, got[o:o + x.nbytes].view(np.float32), x, f'{what} {i} ({x.size} elements)')
    assert (got[~covered] == GUARD).all(), f'guard bytes around the {what}s were written'


def _start_residual(n, seed):
    """A non-zero starting residual: about half a bf16 ulp of a unit-scale value, both signs."""
    return (random_input(DT_FLOAT, n, seed) * np.float32(2.0 ** -9)).astype(np.float32)


@pytest.mark.parametrize('geometry', list(GEOMETRIES))
@pytest.mark.parametrize('wire', WIRES, ids=lambda d: WIRE_NAME[d])
def test_pack_fb_is_the_cpu_model(lib, gpu, wire, geometry):
    lens, bare, tmis, rmis = GEOMETRIES[geometry]
    k = len(lens)
    has = [n > 0 and i not in bare for i, n in enumerate(lens)]
    toffs, ttotal = _tensor_layout(lens, tmis)
    roffs, rtotal = _tensor_layout(lens, rmis)
    foffs, ftotal = _flat_layout(lens)
    resid = [_start_residual(n, 8100 + i) if has[i] else None for i, n in enumerate(lens)]
    res = torch.from_numpy(_guarded(resid, roffs, rtotal)).to(gpu)
    assert res.data_ptr() % 16 == 0
    R = _ptrs(res.data_ptr(), roffs, has)
    for launch in range(2):  # the second launch starts from the residuals the first one left
        data = [wire_input(n, 8000 + 100 * launch + i) for i, n in enumerate(lens)]  # SPECIALS in every head
        thost = _guarded(data, toffs, ttotal)
        src = torch.from_numpy(thost).to(gpu)
        flat = torch.full((ftotal + 2 * FLAT_GUARD,), GUARD, dtype=torch.uint8, device=gpu)
        assert src.data_ptr() % 16 == 0 and flat.data_ptr() % 256 == 0
        st = lib.ddl_pack_cvt_fb(flat.data_ptr() + FLAT_GUARD, _ptrs(src.data_ptr(), toffs, [True] * k), R,
                                 (ctypes.c_size_t * k)(*lens), k, wire, _stream())
        assert st == 0, lib.ddl_last_error()
        torch.cuda.synchronize()
        want = [step_or_cast(wire, x, r) for x, r in zip(data, resid)]
        got = flat.cpu().numpy()
        assert (got[:FLAT_GUARD] == GUARD).all() and (got[FLAT_GUARD + ftotal:] == GUARD).all(), \
            'guard bytes before / after the flat buffer were written'
        got = got[FLAT_GUARD:FLAT_GUARD + ftotal]
        covered = np.zeros(ftotal, bool)
        for i, ((w, _), o) in enumerate(zip(want, foffs)):
            covered[o:o + w.nbytes] = True
            assert_same(wire, got[o:o + w.nbytes].view(w.dtype), w,
                        f'launch {launch} segment {i} ({lens[i]} elements, residual {has[i]})')
        assert (got[~covered] == GUARD).all(), 'padding of the flat buffer was written'
        resid = [r for _, r in want]
        _check_guarded(res.cpu().numpy(), resid, roffs, f'launch {launch} residual')
        assert src.cpu().numpy().tobytes() == thost.tobytes(), 'the pack wrote to its source'
    assert any(r is not None and np.count_nonzero(r) for r in resid)  # (the case is not vacuous)


@pytest.mark.parametrize('wire', WIRES, ids=lambda d: WIRE_NAME[d])
def test_no_residual_is_the_plain_converting_pack(lib, gpu, wire):
    """With every residual NULL the launch is ddl_pack_cvt's: the same bytes, padding included."""
    lens, _, tmis, _ = GEOMETRIES['edges_a']
    k = len(lens)
    data = [wire_input(n, 8500 + i) for i, n in enumerate(lens)]
    toffs, ttotal = _tensor_layout(lens, tmis)
    src = torch.from_numpy(_guarded(data, toffs, ttotal)).to(gpu)
    _, ftotal = _flat_layout(lens)
    S, N = _ptrs(src.data_ptr(), toffs, [True] * k), (ctypes.c_size_t * k)(*lens)
    a = torch.full((ftotal,), GUARD, dtype=torch.uint8, device=gpu)
    b = torch.full((ftotal,), GUARD, dtype=torch.uint8, device=gpu)
    assert lib.ddl_pack_cvt(a.data_ptr(), S, N, k, wire, _stream()) == 0, lib.ddl_last_error()
    assert lib.ddl_pack_cvt_fb(b.data_ptr(), S, (ctypes.c_void_p * k)(*[None] * k), N, k, wire, _stream()) == 0, \
        lib.ddl_last_error()
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_bad_arguments_are_refused(lib, gpu):
    x = torch.zeros(16, dtype=torch.float32, device=gpu)
    one, n1 = (ctypes.c_void_p * 1)(x.data_ptr()), (ctypes.c_size_t * 1)(8)
    assert lib.ddl_pack_cvt_fb(x.data_ptr(), one, one, n1, 1, DT_FLOAT, _stream()) == 4  # UNSUPPORTED_DTYPE
    assert lib.ddl_pack_cvt_fb(x.data_ptr(), one, None, n1, 1, WIRES[0], _stream()) == 3  # INVALID_ARGUMENT
    odd = (ctypes.c_void_p * 1)(x.data_ptr() + 2)  # a residual that is not 4-byte aligned
    assert lib.ddl_pack_cvt_fb(x.data_ptr(), one, odd, n1, 1, WIRES[0], _stream()) == 3
