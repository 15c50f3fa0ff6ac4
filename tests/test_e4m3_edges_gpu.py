"""The kernels of the e4m3 wire on constructed inputs (tests/_e4m3_edge_helpers.py; what they cover is asserted in
tests/test_e4m3_edges_cpu.py), bit for bit against the CPU model of _e4m3_helpers.py / _e4m3_feedback_helpers.py:
  A  k_foldq on every pair of codes under 29 pairs of scales, and the order of its additions;
  B  every k_foldq<NB, FV> instantiation, the tile edges, the size rule between the two variants, a batch;
  C  the pack's scale at every exponent and with the granule's maximum in every slot, an overflowing and an
     underflowing prescale;
  D  the unpack of every code under every scale dword;
  E  the feedback pack on ties, at the scale boundary and at an overflow that only the residual produces."""
import ctypes

import numpy as np
import pytest
import torch

import _e4m3_edge_helpers as eh
import _e4m3_feedback_helpers as fb
import _e4m3_helpers as q8
from _avg_helpers import assert_same
from _helpers import DT_FLOAT
from _sumsq_helpers import mirror
from test_e4m3_feedback_kernel_gpu import _assert_bytes, _pack_fb
from test_e4m3_kernel_gpu import _assert_granules

pytestmark = pytest.mark.gpu
GUARD = 0xA5
VP, SZ = ctypes.c_void_p, ctypes.c_size_t
F = np.float32
THIRD = float(F(1) / F(3))
INVALID_ARGUMENT = 3  # DDL_STATUS_INVALID_ARGUMENT
DTYPE_E4M3, FOLD_LEFT = 0x1e43, 0  # csrc/common.h kDtypeE4m3, kFoldLeft


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _scales(wire):
    return wire.reshape(-1, 256)[:, 252:].copy().view(F).ravel()


# ---- the fold ----------------------------------------------------------------------------------------------------------
@pytest.fixture
def fold_variant(lib):
    """Forces k_foldq's cache-policy variant (process-wide state) and puts the size rule back, also behind a failure."""
    def force(v):
        assert lib.ddl_testing_fold_variant(v) == 0, lib.ddl_last_error()
    yield force
    assert lib.ddl_testing_fold_variant(-1) == 0, lib.ddl_last_error()


def _fold(lib, gpu, ins, what):
    """ddl_fold_e4m3 over ins[0] and the nb = len(ins) - 1 inputs behind it against the model: 256 guard bytes behind
    the output, the inputs not written."""
    ng, nb = ins[0].size // 256, len(ins) - 1
    dev = [torch.from_numpy(w).to(gpu) for w in ins]
    out = torch.full((ng * 256 + 256,), GUARD, dtype=torch.uint8, device=gpu)
    st = lib.ddl_fold_e4m3(out.data_ptr(), dev[0].data_ptr(), (VP * nb)(*[t.data_ptr() for t in dev[1:]]), nb, ng,
                           _stream())
    assert st == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[ng * 256:] == GUARD).all(), f'{what}: the fold wrote past its output'
    for t, w in zip(dev, ins):
        assert t.cpu().numpy().tobytes() == w.tobytes(), f'{what}: the fold wrote to an input'
    _assert_granules(got[:ng * 256], q8.fold(ins), what)


@pytest.mark.parametrize('e0,d', eh.PAIR_CASES, ids=[f'e{e}d{d}' for e, d in eh.PAIR_CASES])
def test_fold_on_every_pair_of_codes(lib, gpu, e0, d):
    """A. All 65 536 pairs of codes, input 0 under the scale bits e0 << 23 and input 1 under (e0 + d) << 23, in the
    natural, a shuffled and the sorted arrangement (homogeneous granules with the tightest scale / a near-maximal sum
    in nearly every granule and the small sums on a coarse grid)."""
    for how in eh.ARRANGEMENTS:
        _fold(lib, gpu, eh.pair_wires(e0, d, how), f'e0 = {e0}, d = {d}, {how}')


@pytest.mark.parametrize('d', eh.ORDER_GAPS)
def test_fold_adds_left_to_right(lib, gpu, d):
    """A. (B, A, -A) with B d binades below A, nb = 2: ((B + A) - A) is B's rounding remainder; the reverse order or a
    tree gives B itself (test_e4m3_edges_cpu.py: both differ from the model here)."""
    _fold(lib, gpu, eh.order_inputs(d), f'(B, A, -A), d = {d}')


@pytest.mark.parametrize('variant', [4, 5])
@pytest.mark.parametrize('nb', range(1, 16))
def test_every_fold_instantiation(lib, gpu, fold_variant, nb, variant):
    """B. k_foldq<nb, variant> on the crafted granules of test_e4m3_kernel_gpu.py (29 granules: three whole 2 KiB
    tiles and a partial one)."""
    fold_variant(variant)
    _fold(lib, gpu, eh.crafted_inputs(nb + 1, 29, 70 + nb), f'nb = {nb}, variant {variant}')


@pytest.mark.parametrize('variant', [4, 5])
@pytest.mark.parametrize('nb', [1, 15])
def test_fold_tile_edges(lib, gpu, fold_variant, nb, variant):
    """B. One granule, one short of / exactly / one past a tile of 8 granules, two tiles, three and a partial one:
    the bound of the tile's buffer descriptor."""
    fold_variant(variant)
    for ng in (1, 7, 8, 9, 16, 29):
        _fold(lib, gpu, eh.crafted_inputs(nb + 1, ng, 30 + nb), f'nb = {nb}, variant {variant}, {ng} granules')


def test_fold_size_rule(lib, gpu):
    """B. Unforced, 16 388 granules: just over the 4 MiB up to which the plain-load variant runs (2 048 whole tiles
    and half a tile)."""
    ng = 16_388
    assert ng * 256 > 4 << 20 and (ng - 8) * 256 <= 4 << 20 and ng % 8 == 4
    ins = [q8.pack(q8.rank_input(ng * q8.G - 7, 55, r)) for r in range(2)]
    _fold(lib, gpu, ins, f'{ng} granules')


def _fold_batch(lib, gpu, tables, nb, order=FOLD_LEFT, out_shift=0):
    """ddl_reduce_fold_batch over the e4m3 granules of tables[i] (nb + 1 inputs each): the status, the outputs (with
    256 guard bytes behind each; an empty table gets an allocation of guard bytes only) and whether an input changed."""
    k = len(tables)
    ngs = [t[0].size // 256 for t in tables]
    dev = [[torch.from_numpy(w).to(gpu) if w.size else torch.full((256,), GUARD, dtype=torch.uint8, device=gpu)
            for w in t] for t in tables]
    outs = [torch.full((ng * 256 + 256 + 16,), GUARD, dtype=torch.uint8, device=gpu) for ng in ngs]
    st = lib.ddl_reduce_fold_batch(k, (VP * k)(*[o.data_ptr() + out_shift for o in outs]),
                                   (VP * k)(*[t[0].data_ptr() for t in dev]),
                                   (VP * (k * nb))(*[x.data_ptr() for t in dev for x in t[1:]]), nb, (SZ * k)(*ngs),
                                   DTYPE_E4M3, order, _stream())
    torch.cuda.synchronize()
    for t, d in zip(tables, dev):
        for w, x in zip(t, d):
            assert not w.size or x.cpu().numpy().tobytes() == w.tobytes(), 'the fold wrote to an input'
    return st, [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize('variant', [4, 5])
def test_fold_batch_of_unequal_tables(lib, gpu, fold_variant, variant):
    """B. Eight tables (kMaxFoldBatch) in one launch, nb = 3: the grid is the longest table's (64 granules, 8 tiles),
    the workgroups past a shorter table's end return early; the empty table's output is untouched."""
    fold_variant(variant)
    nb = 3
    tables = eh.batch_inputs(nb + 1, 200)
    st, outs = _fold_batch(lib, gpu, tables, nb)
    assert st == 0, lib.ddl_last_error()
    for i, (t, got, ng) in enumerate(zip(tables, outs, eh.BATCH_GRANULES)):
        assert (got[ng * 256:] == GUARD).all(), f'table {i}: the fold wrote past its output'
        if ng:
            _assert_granules(got[:ng * 256], q8.fold(t), f'table {i} ({ng} granules), variant {variant}')


def test_fold_batch_refusals(lib, gpu):
    """B. An output that is only 4-byte aligned and every order but the left one are refused before anything runs."""
    nb = 3
    tables = eh.batch_inputs(nb + 1, 200)[:2]
    for what, kw in [('output off by 4 bytes', dict(out_shift=4)), ('the MPICH tree order', dict(order=1)),
                     ('the binomial order', dict(order=2)), ('no order at all', dict(order=7))]:
        st, outs = _fold_batch(lib, gpu, tables, nb, **kw)
        assert st == INVALID_ARGUMENT, what
        assert all((o == GUARD).all() for o in outs), f'{what}: something ran'
    st, _ = _fold_batch(lib, gpu, tables, nb)
    assert st == 0, lib.ddl_last_error()  # the same call without the defect


# ---- the pack --------------------------------------------------------------------------------------------------------
def _layout(lens, shifts):
    """Byte offsets of arrays of lens[i] 4-byte elements inside one guarded allocation: array i 16-byte aligned plus
    shifts[i] bytes, 48 guard bytes behind each."""
    offs, cur = [], 64
    for n, sh in zip(lens, shifts):
        cur = ((cur + 15) & ~15) + sh
        offs.append(cur)
        cur += 4 * n + 48
    return offs, cur + 64


def _pack(lib, gpu, data, shifts, scale=None):
    """One ddl_pack_e4m3 launch over the segments `data`, segment i shifts[i] bytes past a 16-byte boundary; guard
    bytes around the flat buffer, the source not written. Returns the flat buffer's bytes per segment."""
    lens = [x.size for x in data]
    k = len(lens)
    toffs, ttotal = _layout(lens, shifts)
    host = np.full(ttotal, GUARD, np.uint8)
    for x, o in zip(data, toffs):
        host[o:o + x.nbytes] = x.view(np.uint8)
    src = torch.from_numpy(host).to(gpu)
    foffs, ftotal = q8.flat_layout(lens)
    flat = torch.full((ftotal + 512,), GUARD, dtype=torch.uint8, device=gpu)  # 256 guard bytes on either side
    st = lib.ddl_pack_e4m3(flat.data_ptr() + 256, (VP * k)(*[src.data_ptr() + o for o in toffs]), (SZ * k)(*lens), k,
                           (ctypes.c_float * k)(*scale) if scale else None, _stream())
    assert st == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    got = flat.cpu().numpy()
    assert (got[:256] == GUARD).all() and (got[256 + ftotal:] == GUARD).all(), 'the pack wrote outside the flat buffer'
    assert src.cpu().numpy().tobytes() == host.tobytes(), 'the pack wrote to its source'
    return [got[256 + o:256 + o + q8.granules(n) * 256] for o, n in zip(foffs, lens)]


def _split(x, cuts):
    """fp32[granules, 252] -> segments of whole granules, cut at the granule indexes `cuts`."""
    edges = [0] + list(cuts) + [x.shape[0]]
    return [np.ascontiguousarray(x[a:b]).ravel() for a, b in zip(edges, edges[1:])]


def test_pack_scale_at_every_exponent(lib, gpu):
    """C. A granule maximum at E = 1..254 with the mantissas around 1.75 (the last one of a scale), at 0 and among the
    subnormals, in slot (granule index) % 252, the rest of the granule ties of the scale the model assigns: the scale
    dword and the codes. Five segments of one launch, two of them only 4-byte aligned."""
    data = _split(eh.exponent_granules(), (1, 254, 700, 1001))
    got = _pack(lib, gpu, data, [0, 4, 0, 12, 8])
    for i, (x, g) in enumerate(zip(data, got)):
        _assert_granules(g, q8.pack(x), f'segment {i} ({x.size // 252} granules)')


@pytest.mark.parametrize('specials', [False, True], ids=['finite', 'nan_inf_beside'])
def test_pack_scale_from_every_slot(lib, gpu, specials):
    """C. Granule p has its only large element in slot p (+-2**-140 elsewhere; with `specials` a NaN and an infinity
    beside it): the scale comes from that element alone, whichever lane and register of the row reduction holds it."""
    x, big = eh.slot_granules(specials)
    data = _split(x, (100,))
    got = np.concatenate(_pack(lib, gpu, data, [4, 0]))
    want = q8.pack(x.ravel())
    assert np.array_equal(_scales(want), np.abs(big) / F(448))
    bad = np.flatnonzero(_scales(got).view(np.uint32) != _scales(want).view(np.uint32))
    assert bad.size == 0, f'the scale of the granules with the maximum in slots {bad.tolist()} differs'
    _assert_granules(got, want, 'every slot')


def test_pack_prescale_overflow_and_underflow(lib, gpu):
    """C. +-1e38 times 4.0: every product is infinite, so every code is 0x7f | sign and the scale 2**-126; 2**-120
    times 2**-20: the products are fp32 subnormals, below half the smallest code; (1..8) * 2**-110 times 2**-20:
    subnormal products that have codes."""
    n = 1009
    huge = np.where(np.arange(n) % 3 == 0, F(-1e38), F(1e38)).astype(F)
    small = np.where(np.arange(n) % 5 == 0, F(-2.0 ** -120), F(2.0 ** -120)).astype(F)
    coded = (small * np.ldexp(F(1), 10 + np.arange(n) % 4)).astype(F) * (1 + np.arange(n) % 2).astype(F)
    got = _pack(lib, gpu, [huge, small, huge, coded], [0, 4, 4, 0], [4.0, 2.0 ** -20, 4.0, 2.0 ** -20])
    want = [q8.pack(huge, 4.0), q8.pack(small, 2.0 ** -20), q8.pack(huge, 4.0), q8.pack(coded, 2.0 ** -20)]
    w = want[0].reshape(-1, 256)
    assert (_scales(want[0]) == F(2.0 ** -126)).all()
    assert np.array_equal(w[:, :252].ravel()[:n], np.where(np.arange(n) % 3 == 0, 0xff, 0x7f))
    assert (_scales(want[1]) == F(2.0 ** -126)).all() and set(want[1].reshape(-1, 256)[0, :252].tolist()) == {0x00, 0x80}
    assert (_scales(want[3]) == F(2.0 ** -126)).all() and (want[3].reshape(-1, 256)[0, :252] & 0x7f).min() >= 0x18
    for i, (g, wnt) in enumerate(zip(got, want)):
        _assert_granules(g, wnt, f'segment {i}')


# ---- the unpack ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('post', [1.0, THIRD], ids=['plain', 'postscale'])
@pytest.mark.parametrize('P', [3, 7, 16])
def test_unpack_under_every_scale(lib, gpu, P, post):
    """D. Every code under every scale exponent byte, a non-power-of-two, a negative, a NaN and two subnormal scales:
    each segment once as SUM and once as AVG over P in one launch, 16-byte and 4-byte aligned in turn, with and without
    the sum of squares (asked for where the expected output has no NaN: the segments of the codes 0..126)."""
    segs = eh.unpack_segments()
    wires = [w for w, _ in segs] * 2
    lens = [n for _, n in segs] * 2
    ops = [q8.OP_SUM] * len(segs) + [q8.OP_AVG] * len(segs)
    k = len(lens)
    want = [q8.unpack(w, n, op, P, post) for w, n, op in zip(wires, lens, ops)]
    want_stat = [0 if np.isnan(y).any() else 1 for y in want]
    assert sum(want_stat) == 2 * (len(segs) - 4)
    foffs, ftotal = q8.flat_layout(lens)
    fhost = np.full(ftotal, 0x5A, np.uint8)
    for w, o in zip(wires, foffs):
        fhost[o:o + w.size] = w
    flat = torch.from_numpy(fhost).to(gpu)
    toffs, ttotal = _layout(lens, [4 * ((i + i // len(segs)) % 2) for i in range(k)])
    for stat in (False, True):
        dst = torch.full((ttotal,), GUARD, dtype=torch.uint8, device=gpu)
        sums = (ctypes.c_double * k)()
        st = lib.ddl_unpack_e4m3((VP * k)(*[dst.data_ptr() + o for o in toffs]), flat.data_ptr(), (SZ * k)(*lens),
                                 (ctypes.c_int * k)(*ops), k, P, (ctypes.c_float * k)(*[post] * k) if post != 1.0 else None,
                                 _stream(), (ctypes.c_ubyte * k)(*want_stat) if stat else None, sums if stat else None)
        assert st == 0, lib.ddl_last_error()
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        covered = np.zeros(ttotal, bool)
        for i, (y, o) in enumerate(zip(want, toffs)):
            covered[o:o + y.nbytes] = True
            what = f'segment {i} ({lens[i]} elements, {"AVG" if ops[i] else "SUM"}, statistic {stat})'
            assert_same(DT_FLOAT, got[o:o + y.nbytes].view(F), y, what)
            if stat:
                s = mirror(y, compressed=False) if want_stat[i] else 0.0
                assert np.float64(sums[i]).tobytes() == np.float64(s).tobytes(), 'sum of squares of ' + what
        assert (got[~covered] == GUARD).all(), 'bytes outside the segments were written'
        assert flat.cpu().numpy().tobytes() == fhost.tobytes(), 'the unpack wrote to the flat buffer'


# ---- the feedback pack -----------------------------------------------------------------------------------------------
def _exact_residual(x, r, wire):
    """fp64(v) - fp64(code * s) from the wire that came back, v = x (+) r in fp32; +0.0 behind a NaN or an infinity,
    in v or in what was sent for it (code * s as the fold and the unpack read it, in fp32). Must be an fp32."""
    with np.errstate(all='ignore'):
        v = (x + r).astype(F)
    w = wire.reshape(-1, 256)
    d = (q8.DECODE[w[:, :252]].astype(np.float64) * _scales(wire).astype(np.float64)[:, None]).ravel()[:v.size]
    with np.errstate(all='ignore'):
        fin = np.isfinite(v) & np.isfinite(d.astype(F))
    e = np.zeros(v.size, np.float64)
    e[fin] = v[fin].astype(np.float64) - d[fin]
    assert np.array_equal(e.astype(F).astype(np.float64), e), 'the exact residual is not an fp32'
    return e.astype(F)


@pytest.mark.parametrize('exp', eh.FB_SCALE_EXPONENTS)
def test_feedback_pack_at_the_edges(lib, gpu, exp):
    """E. Under the scale 2**exp, one launch of three segments and a second one chained to its residuals:
    0 every tie of the format and its fp32 neighbours with zero residuals: ddl_pack_e4m3's bytes (but for -0.0, which
      -0.0 (+) +0.0 makes +0.0), and the residual is fp64(v) - fp64(decoded) exactly;
    1 the code values with residuals of half a code spacing (ties that only the residual produces), and a granule
      whose maximum 448 s gets a residual of one ulp: the scale doubles;
    2 FLT_MAX with the residual FLT_MAX among ties: code 0x7f, residual +0.0, the granule's scale unchanged; in the
      second launch FLT_MAX alone: finite, but sent as 256 * 2**120, an infinity in fp32, so the residual is +0.0."""
    s = np.ldexp(F(1), exp)
    x0 = eh.sweep_values(s)
    cases = [(x0, np.zeros(x0.size, F)), eh.fb_tie_case(s), eh.fb_overflow_case(s)]
    data, res = [c[0] for c in cases], [c[1] for c in cases]
    k = len(data)
    for step in range(2):
        got, foffs, rgot = _pack_fb(lib, gpu, data, res, [True] * k, misaligned=step == 1)
        for i, (x, r, o) in enumerate(zip(data, res, foffs)):
            want, rwant = fb.pack_fb(x, r)
            wire = got[o:o + want.size]
            _assert_bytes(wire, want, f'step {step} segment {i} wire')
            _assert_bytes(rgot[i], rwant, f'step {step} segment {i} residual')
            _assert_bytes(rgot[i], _exact_residual(x, r, wire), f'step {step} segment {i} residual against fp64')
        if step == 0:
            plain = _pack_fb(lib, gpu, data, res, [False] * k, False, plain=True)[0]
            n0 = q8.granules(x0.size) * 256
            # (-0.0 (+) +0.0 is +0.0: the one input whose code a zero residual changes, 0x80 -> 0x00, by the rule)
            zero = np.flatnonzero(x0.view(np.uint32) == 0x80000000)
            at = zero // 252 * 256 + zero % 252
            assert zero.size == 1 and plain[at] == 0x80 and got[at] == 0x00
            plain[at] = 0x00
            _assert_bytes(got[:n0], plain[:n0], "zero residuals against ddl_pack_e4m3's bytes")
            assert (_scales(got[:n0]) == s).all()
            bad = ~np.isfinite(x0)
            assert bad.sum() == 4 and not rgot[0][bad].view(np.uint32).any()  # +0.0 behind NaN and +-inf
            t = got[foffs[1]:foffs[2]]
            assert (_scales(t)[:-1] == s).all() and _scales(t)[-1] == (2 * s if exp != 120 else s)
            o = got[foffs[2]:]
            assert o[100] == 0x7f and rgot[2][100].view(np.uint32) == 0 and (_scales(o) == s).all()
        else:  # FLT_MAX, now with a residual of 0: finite, sent as 256 * 2**120 = +inf in fp32: nothing is kept
            o = got[foffs[2]:]
            assert o[100] == 0x78 and _scales(o)[0] == F(2.0 ** 120) and rgot[2][100].view(np.uint32) == 0
        # the next step: the same gradients on the residuals the GPU returned (a tie's half spacing among them)
        res = rgot
