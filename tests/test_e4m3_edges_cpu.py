"""What the constructed inputs of tests/_e4m3_edge_helpers.py cover, computed with the model alone, so that the inputs
of tests/test_e4m3_edges_gpu.py cannot decay unnoticed: every output code, ties and inexact additions in the fold on
every pair of codes; wrong engines (and wrong orders of addition) that must each differ from the model on those
inputs; the scale rule's edges among the pack's granules; fp32-subnormal products and a flush-to-zero decoder on the
unpack's wire; the ties and the scale boundary that only a residual produces."""
import numpy as np
import pytest

import _e4m3_edge_helpers as eh
import _e4m3_feedback_helpers as fb
import _e4m3_helpers as q8
from test_e4m3_kernel_gpu import _sweep_values
from test_e4m3_model_cpu import _mx_scale, _saturating_rne, _trunc_codes

F = np.float32
TINY = F(2.0 ** -126)  # the smallest normal fp32


def _codes(wire):
    return wire.reshape(-1, 256)[:, :252]


def _scales(wire):
    return wire.reshape(-1, 256)[:, 252:].copy().view(F).ravel()


# ---- A ---------------------------------------------------------------------------------------------------------------
def test_the_pair_cases_are_the_issues():
    assert len(eh.PAIR_CASES) == len(set(eh.PAIR_CASES)) == 29
    assert sorted(d for e, d in eh.PAIR_CASES if e == 127) == sorted(
        [0] + [s * g for g in (1, 2, 3, 4, 5, 8, 9, 13, 21, 25) for s in (1, -1)])
    assert [c for c in eh.PAIR_CASES if c[0] == 1] == [(1, 0), (1, 1), (1, 4)]
    assert sorted(d for e, d in eh.PAIR_CASES if e == 247) == [-4, -1, 0, 1, 4]
    assert all(1 <= e + d <= 254 for e, d in eh.PAIR_CASES)  # normal, finite scales
    w0, w1 = eh.pair_wires(127, 3)
    assert w0.size == w1.size == 261 * 256 and eh.PAIR_GRANULES == 261
    k = np.arange(eh.PAIRS)
    assert np.array_equal(_codes(w0).ravel()[:eh.PAIRS], k >> 8) and np.array_equal(_codes(w1).ravel()[:eh.PAIRS], k & 255)
    assert not _codes(w0).ravel()[eh.PAIRS:].any() and not _codes(w1).ravel()[eh.PAIRS:].any()
    assert (_scales(w0) == 1.0).all() and (_scales(w1) == 8.0).all()
    for how in ('shuffled', 'sorted'):  # the same 65 536 pairs, each once
        a, b = eh.pair_wires(127, 3, how)
        pair = _codes(a).ravel()[:eh.PAIRS].astype(np.int64) << 8 | _codes(b).ravel()[:eh.PAIRS]
        assert np.array_equal(np.sort(pair), k) and not np.array_equal(pair, k)
    for e0, d in ((127, 3), (247, 1)):  # sorted: |sum| ascending, a NaN as 0, the infinities last
        m = np.abs(eh.pair_sums(e0, d)[0][eh._pair_order(e0, d, 'sorted')]).astype(np.float64)
        nan = np.isnan(m)
        m[nan] = 0.0
        assert (m[1:] >= m[:-1]).all()
    assert np.isinf(m[-1]) and nan.any()


def _midpoints():
    d = q8.DECODE[:0x7f].astype(np.float64)
    return ((d[:-1] + d[1:]) / 2).astype(F)


def test_fold_pairs_reach_every_code_tie_and_inexact_sum():
    """The coverage conditions of the 29 x 3 cases. The rarest code appeared 5 069 times, 0x80 5 360 times, 0xff (a
    negative overflow) 71 730 times, 377 205 ties and 502 998 inexact additions when this was written; the thresholds
    are what the inputs must keep."""
    hist = np.zeros(256, np.int64)
    ties = inexact = elements = 0
    mid = _midpoints()
    for e0, d in eh.PAIR_CASES:
        s32, s64 = eh.pair_sums(e0, d)
        fin = np.isfinite(s32)
        inexact += 3 * int(np.count_nonzero(s32[fin].astype(np.float64) != s64[fin]))
        for how in eh.ARRANGEMENTS:
            out = q8.fold(eh.pair_wires(e0, d, how))
            elements += out.size // 256 * 252
            hist += np.bincount(_codes(out).ravel()[:eh.PAIRS], minlength=256)
            sums = s32[eh._pair_order(e0, d, how)]
            sums = np.concatenate([sums, np.zeros(eh.PAIR_GRANULES * 252 - eh.PAIRS, F)]).reshape(-1, 252)
            with np.errstate(all='ignore'):
                y = np.abs(sums / _scales(out)[:, None]).astype(F)  # exact: the scale is a power of two
            ties += int(np.count_nonzero(np.isin(y, mid) & np.isfinite(sums)))
    assert elements == 87 * 261 * 252 == 5_722_164
    assert hist.min() >= 1000, (int(hist.argmin()), int(hist.min()))  # every one of the 256 output codes, and often
    assert hist[0x80] >= 1000 and hist[0xff] >= 1000 and hist[0x7f] >= 1000
    assert ties >= 100_000, ties
    assert inexact >= 100_000, inexact


def _ties_away(y):
    """Round to nearest, ties away from zero."""
    y = np.ascontiguousarray(y, F)
    d = q8.DECODE[:0x7f].astype(np.float64)
    mag = np.abs(y).astype(np.float64)
    lo = np.clip(np.searchsorted(d, mag, side='right') - 1, 0, 0x7e)
    hi = np.minimum(lo + 1, 0x7e)
    code = np.where(mag - d[lo] >= d[hi] - mag, hi, lo)
    return (code.astype(np.uint8) | ((y.view(np.uint32) >> 24).astype(np.uint8) & 0x80)).astype(np.uint8)


def _flush(x):
    return np.where(np.abs(x) < TINY, F(0) * x, x).astype(F)  # (the sign kept, as the hardware mode does)


def _fold_with(wires, flush_products=False, flush_sums=False, keep_nan_sign=False, order='left', **q):
    """q8.fold with one thing wrong."""
    with np.errstate(all='ignore'):
        xs = [q8.dequantize(w) for w in wires]
        if flush_products:
            xs = [_flush(x) for x in xs]
        if order == 'reverse':
            xs = xs[::-1]
        if order == 'tree':  # x_0 + (x_1 + x_2)
            assert len(xs) == 3
            y = (xs[0] + (xs[1] + xs[2]).astype(F)).astype(F)
        else:
            y = xs[0]
            for x in xs[1:]:
                y = (y + x).astype(F)
        if flush_sums:
            y = _flush(y)
    if not keep_nan_sign:
        y[np.isnan(y)] = F(np.nan)
    return q8.quantize(y, **q)


def _first_difference(how=('natural',), cases=eh.PAIR_CASES, **wrong):
    for e0, d in cases:
        for h in how:
            w = eh.pair_wires(e0, d, h)
            if _fold_with(w, **wrong).tobytes() != q8.fold(w).tobytes():
                return e0, d, h
    return None


def test_wrong_engines_differ_on_the_fold_pairs():
    w = eh.pair_wires(127, 0)
    assert _fold_with(w).tobytes() == q8.fold(w).tobytes()  # the comparison itself: nothing wrong, nothing differs
    assert _first_difference(rne=_trunc_codes), 'truncation'
    assert _first_difference(rne=_ties_away), 'ties away from zero'
    sub = [c for c in eh.PAIR_CASES if c[0] == 1]
    assert _first_difference(cases=sub, flush_products=True), 'products flushed to zero'
    assert _first_difference(cases=sub, flush_sums=True), 'sums flushed to zero'
    over = [c for c in eh.PAIR_CASES if c[0] == 247]
    assert _first_difference(cases=over, finite_amax=False), 'amax over non-finite sums'
    assert _first_difference(keep_nan_sign=True), 'the sign of a NaN sum kept'
    assert _first_difference(scale=_mx_scale, rne=_saturating_rne), 'a saturating quantizer with the MX scale rule'
    # ties away and truncation are told apart from RNE by ties alone in the sorted arrangement, too
    assert _first_difference(how=('sorted',), cases=[(127, 1)], rne=_ties_away)
    # the ordinary cases hold no fp32 subnormal: a flush there changes nothing (what the e0 = 1 cases are for)
    assert _first_difference(cases=[(127, 0), (127, -25)], flush_products=True, flush_sums=True) is None


@pytest.mark.parametrize('d', eh.ORDER_GAPS)
def test_wrong_orders_of_addition_differ(d):
    """(B, A, C) with C = -A: left to right the fold gives B's rounding remainder against A, the reverse order and
    the tree x_0 + (x_1 + x_2) give B itself."""
    ins = eh.order_inputs(d)
    b, a, c = (q8.dequantize(w) for w in ins)
    fin = np.isfinite(a) & np.isfinite(b)
    assert np.array_equal(c[fin], -a[fin])
    want = q8.fold(ins)
    assert _fold_with(ins).tobytes() == want.tobytes()
    for order in ('reverse', 'tree'):
        got = _fold_with(ins, order=order)
        assert got.tobytes() != want.tobytes(), order
        back = q8.dequantize(got)
        assert np.array_equal(back[fin], b[fin])  # B itself: exact, requantized under its own scale
    lost = q8.dequantize(want)[fin] != b[fin]
    assert np.count_nonzero(lost) >= 1000  # the order shows in many elements, not in a corner


# ---- B ---------------------------------------------------------------------------------------------------------------
def test_crafted_inputs_keep_their_crafted_granules_at_every_size():
    for ng in (1, 7, 8, 9, 16, 29):
        ins = eh.crafted_inputs(3, ng, 5)
        assert all(w.size == ng * 256 for w in ins)
        assert not ins[0][:256].any() or ng == 29  # the all-zero granule (a zero scale) comes first
        if 7 <= ng < 29:
            assert np.isnan(_scales(ins[2])[5])  # the NaN scale
            assert (_scales(ins[0])[2] == F(2.0 ** 120)) and (_scales(ins[0])[3] == TINY)
    tables = eh.batch_inputs(4, 9)
    assert [w[0].size // 256 for w in tables] == eh.BATCH_GRANULES == [29, 1, 0, 8, 9, 64, 7, 3]
    assert all(len(t) == 4 for t in tables)


# ---- C ---------------------------------------------------------------------------------------------------------------
def test_sweep_values_extend_the_kernel_tests():
    for exp in (-126, 0, 100):
        s = np.ldexp(F(1), exp)
        assert eh.sweep_values(s).tobytes() == _sweep_values(s).tobytes()
    for exp in eh.FB_SCALE_EXPONENTS:
        s = np.ldexp(F(1), exp)
        x = eh.sweep_values(s)
        w = q8.pack(x)
        assert (_scales(w) == s).all()
        codes = _codes(w).ravel()[:x.size]
        assert set(codes.tolist()) >= set(range(0, 0x78)) | {0x7f, 0x80, 0xff}  # (2**120: the codes up to FLT_MAX / s)
        assert exp == 120 or set(codes.tolist()) == set(range(256))


def test_exponent_granules_cover_the_scale_rule():
    x = eh.exponent_granules()
    mx = eh.exponent_maxima()
    assert x.shape == (254 * 5 + 3, 252) and np.isfinite(x).all()
    amax = np.abs(x).max(axis=1)
    assert np.array_equal(amax, mx)
    g = np.arange(x.shape[0])
    assert np.array_equal(np.abs(x[g, g % 252]), mx) and (np.count_nonzero(np.abs(x) == mx[:, None], axis=1)[mx > 0] == 1).all()
    assert set((g % 252).tolist()) == set(range(252))  # the maximum visits every slot
    assert (np.signbit(x[g, g % 252]) == (g % 2 == 1)).all()
    w = q8.pack(x.ravel())
    e = (_scales(w).view(np.uint32) >> 23).astype(int)
    assert set(e.tolist()) == set(range(1, 248))  # every scale exponent the rule can give: 2**-126 .. 2**120
    # a scale off by one binade, either way, changes the codes of every granule whose maximum is not 0 (not only the
    # scale dword): the maximum itself codes differently
    for wrong in (lambda a: q8.scale_of(a) * F(2), lambda a: np.maximum(q8.scale_of(a) / F(2), TINY)):
        bad = q8.pack(x.ravel(), scale=wrong, rne=_saturating_rne)
        differ = (_codes(bad) != _codes(w)).any(axis=1)
        changed = _scales(bad) != _scales(w)
        assert differ[changed & (mx >= TINY)].all() and np.count_nonzero(changed & (mx >= TINY)) >= 1000
    # the rule's own off-by-one: 0x200000 for 0x1fffff moves only a maximum of exactly 1.75 * 2**k, which is here for
    # every k
    u = mx.view(np.uint32).astype(np.int64)
    off = np.maximum(((u + 0x200000) >> 23) - 8, 1) != np.maximum(((u + 0x1fffff) >> 23) - 8, 1)
    assert np.count_nonzero(off) == 246 and (u[off] & 0x7fffff == 0x600000).all()  # (E <= 8: both 2**-126)


def test_slot_granules_have_one_large_element_each():
    for specials in (False, True):
        x, big = eh.slot_granules(specials)
        p = np.arange(252)
        assert np.array_equal(x[p, p], big) and set(np.abs(big).tolist()) == {448.0 * 2.0 ** k for k in range(-20, 20)}
        fin = np.where(np.isfinite(x), np.abs(x), 0)
        assert (np.count_nonzero(fin > F(2.0 ** -140), axis=1) == 1).all()
        assert np.count_nonzero(~np.isfinite(x)) == (504 if specials else 0)
        w = q8.pack(x.ravel())
        assert np.array_equal(_scales(w), np.ldexp(F(1), p % 40 - 20))  # from element p alone
        assert (_codes(w)[p, p] == np.where(p % 2, 0xfe, 0x7e)).all()
        # an amax that misses one slot (a lost step of the row reduction) gives that granule the smallest scale
        assert (q8.scale_of(F(2.0 ** -140)) == TINY)


# ---- D ---------------------------------------------------------------------------------------------------------------
def test_unpack_wire_holds_every_code_under_every_scale():
    w = eh.unpack_wire().reshape(-1, 256)
    assert w.shape[0] == 2 * 261 and len(eh.SCALE_DWORDS) == 261 == len(set(eh.SCALE_DWORDS))
    sc = w[:, 252:].copy().view(np.uint32).ravel()
    for i, dword in enumerate(eh.SCALE_DWORDS):
        assert sc[2 * i] == sc[2 * i + 1] == dword
        both = np.concatenate([w[2 * i, :252], w[2 * i + 1, :4]])
        assert np.array_equal(both, np.arange(256)) and not w[2 * i + 1, 4:252].any()
    y = q8.dequantize(w.ravel()).reshape(-1, 252)
    sub = (np.abs(y) > 0) & (np.abs(y) < TINY)
    assert sub[2].any() and np.count_nonzero(sub) >= 500  # E = 1: fp32-subnormal products (and the subnormal scales')
    with np.errstate(all='ignore'):
        inexact = y.astype(np.float64) != q8.DECODE[w[:, :252]].astype(np.float64) * w[:, 252:].copy().view(F).astype(np.float64)
    assert np.count_nonzero(inexact & np.isfinite(y)) >= 50  # a subnormal scale: the product itself rounds
    assert np.isnan(y[0][0x7f]) and (y[0][:0x7f] == 0).all()  # a zero scale
    assert np.isnan(y[2 * 255][0]) and np.isinf(y[2 * 255][1:0x7f]).all()  # an infinite scale: 0 * inf
    assert np.isnan(y[2 * 258]).all()  # a NaN scale
    assert (y[2 * 257][1:0x7f] < 0).all()  # a negative scale
    segs = eh.unpack_segments()
    assert sum(w.size for w, _ in segs[:4]) == 2 * 261 * 256  # the whole wire
    assert any(n % 252 for _, n in segs[:4]) and all(q8.granules(n) * 256 == w.size for w, n in segs)
    clean = [not np.isnan(q8.unpack(w, n)).any() for w, n in segs]
    assert clean == [False] * 4 + [True] * (len(segs) - 4)


def test_a_flushing_decoder_differs_on_the_unpack_wire():
    w = eh.unpack_wire()
    third = float(F(1) / F(3))
    for op, P, post in [(q8.OP_SUM, 1, 1.0), (q8.OP_AVG, 3, 1.0), (q8.OP_AVG, 16, third)]:
        want = q8.unpack(w, w.size // 256 * 252, op, P, post)
        with np.errstate(all='ignore'):
            y = _flush(q8.dequantize(w))
            if op == q8.OP_AVG:
                y = _flush((y / F(P)).astype(F))
            if post != 1.0:
                y = _flush((y * F(post)).astype(F))
        fin = ~np.isnan(want)
        assert np.array_equal(np.isnan(y), ~fin)
        assert np.count_nonzero(y[fin].view(np.uint32) != want[fin].view(np.uint32)) >= 500


# ---- E ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('exp', eh.FB_SCALE_EXPONENTS)
def test_feedback_cases_are_what_they_say(exp):
    s = np.ldexp(F(1), exp)
    mid = _midpoints()
    # ties that only the residual produces: x is a code value (a fixed point of the pack), x + r is a midpoint
    x, r = eh.fb_tie_case(s)
    assert x.size == r.size
    plain = q8.pack(x)
    body = slice(0, x.size - 201 if exp != 120 else x.size)  # (ahead of the boundary granule)
    assert np.array_equal(q8.dequantize(plain)[:x.size][body], x[body])
    v = (x + r).astype(F)
    assert np.array_equal(v.astype(np.float64), x.astype(np.float64) + r.astype(np.float64))  # exact
    y = np.abs(v[body] / s).astype(F)
    assert np.count_nonzero(np.isin(y, mid)) >= 4 * 100  # (2**120: the codes up to FLT_MAX / s only)
    wire, rn = fb.pack_fb(x, r)
    assert (_scales(wire)[:-1] == s).all()
    if exp != 120:
        assert _scales(plain)[-1] == s and _scales(wire)[-1] == 2 * s  # one ulp of residual doubles the scale
    # a tie leaves a residual of exactly half a spacing: the next step's input
    assert np.count_nonzero(rn) >= 400
    # the overflow
    x, r = eh.fb_overflow_case(s)
    assert x[100] == eh.FLT_MAX and r[100] == eh.FLT_MAX
    wire, rn = fb.pack_fb(x, r)
    assert wire[100] == 0x7f and rn[100] == 0 and not np.signbit(rn[100]) and (_scales(wire) == s).all()
    # the step behind it: FLT_MAX itself, finite, goes out as 256 * 2**120 (an infinity in fp32): nothing is kept, and
    # nothing of it reaches the step after
    wire, rn2 = fb.pack_fb(x, rn)
    assert wire[100] == 0x78 and _scales(wire)[0] == F(2.0 ** 120) and np.isinf(q8.dequantize(wire)[100])
    assert np.isfinite(rn2).all() and rn2[100].view(np.uint32) == 0
