"""Input sets that hold every 16-bit pattern, and their CPU references, for the two-input reduce,
the N-input folds and the converting pack (tests/test_edge_values_cpu.py, test_edge_values_gpu.py).

Everything here runs on the CPU. Expected values are the oracle's (oracle/ddl_oracle.c: sum2, fold,
allreduce_ring / allreduce_direct), cross-checked against a plain numpy restatement (np_fold: fp32
adds, then numpy's cast for fp16 and torch CPU's for bf16, _wire_helpers.narrow); fp32 / fp64 use
numpy's `+`. Never the engine's own output. fp16 arrays are np.float16, bf16 arrays raw np.uint16, as
the other helpers keep them.
"""
import functools

import numpy as np

from _avg_helpers import is_nan
from _helpers import DT_BFLOAT16, DT_DOUBLE, DT_FLOAT, DT_HALF, NP
from _wire_helpers import narrow, widen

HALF_TYPES = [DT_HALF, DT_BFLOAT16]
MANT = {DT_HALF: 10, DT_BFLOAT16: 7}            # stored mantissa bits
INF = {DT_HALF: 0x7c00, DT_BFLOAT16: 0x7f80}    # the inf pattern = the exponent mask
MIN_NORMAL = {DT_HALF: 0x0400, DT_BFLOAT16: 0x0080}

# ±0, ±smallest and ±largest subnormal, ±smallest normal, ±1, ±max, ±inf, a quiet, a signalling and
# a negative NaN, a mid subnormal, a small, a medium and a large normal
FIXED = {
    DT_HALF: [0x0000, 0x8000, 0x0001, 0x8001, 0x03ff, 0x83ff, 0x0400, 0x8400, 0x3c00, 0xbc00, 0x7bff, 0xfbff,
              0x7c00, 0xfc00, 0x7e00, 0x7c01, 0xfe00, 0x0200, 0x1400, 0x3555, 0x6800],
    DT_BFLOAT16: [0x0000, 0x8000, 0x0001, 0x8001, 0x007f, 0x807f, 0x0080, 0x8080, 0x3f80, 0xbf80, 0x7f7f, 0xff7f,
                  0x7f80, 0xff80, 0x7fc0, 0x7f81, 0xffc0, 0x0040, 0x0c00, 0x3eab, 0x7000],
}
N_DERIVED = 5
N_GROUPS = len(FIXED[DT_HALF]) + N_DERIVED       # 26
N_PATTERNS = 1 << 16
N_PAIRS = N_GROUPS * N_PATTERNS                  # 1,703,936

# 7 pairs behind the pair set (n mod 8 = 7: the tail lanes of the vector kernels run), as indices into
# FIXED: max + max (overflow), smallest + smallest subnormal, largest subnormal + smallest subnormal
# (= the smallest normal), inf - inf, signalling NaN + 1, -0 + -0, max - max
TAIL_PAIRS = [(10, 10), (2, 2), (4, 2), (12, 13), (15, 8), (1, 1), (10, 11)]


def patterns():
    return np.arange(N_PATTERNS, dtype=np.uint32).astype(np.uint16)


def storage(dt, bits):
    """uint16 bit patterns as the suite stores the type (np.float16 view / raw uint16)."""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    return bits.view(np.float16) if dt == DT_HALF else bits


def bits_of(x):
    return np.ascontiguousarray(x).view(np.uint16)


def half_ulp(dt, a):
    """Magnitude pattern of half an ulp of a: for exponent field e the power of two with exponent field
    e - (mantissa bits + 1); where that field would be <= 0 the subnormal power of two of the same
    value, and zero where it is not representable (so zero for zeros and subnormals too). inf / NaN
    patterns go by their exponent field like a normal."""
    m = MANT[dt]
    e = ((a.astype(np.int32) & INF[dt]) >> m)
    f = e - (m + 1)
    k = f + m - 1                                   # bit of the subnormal 2^(f - bias), f <= 0
    out = np.where(f >= 1, f << m, np.where(k >= 0, 1 << np.maximum(k, 0), 0))
    return out.astype(np.uint16)


def derived_partners(dt, a):
    """The 5 partners derived from a (uint16 patterns): a, -a, the opposite sign one pattern further
    from zero (cancellation down to one ulp; inf and NaN keep their magnitude), and half an ulp of a
    with a's sign and with the opposite sign (exact ties of the sum)."""
    sign, mag = a & 0x8000, a & 0x7fff
    flip = sign ^ 0x8000
    step = np.where(mag >= INF[dt], mag, mag + 1).astype(np.uint16)
    h = half_ulp(dt, a)
    return [a.copy(), a ^ 0x8000, flip | step, sign | h, flip | h]


@functools.lru_cache(maxsize=None)
def _groups(dt):
    a = patterns()
    gs = [np.full(N_PATTERNS, v, np.uint16) for v in FIXED[dt]] + [g.astype(np.uint16) for g in derived_partners(dt, a)]
    assert len(gs) == N_GROUPS
    return gs


@functools.lru_cache(maxsize=None)
def pair_bits(dt):
    """(A tiled 26 times, the 26 groups of partners) as uint16 patterns, 1,703,936 pairs."""
    a = np.tile(patterns(), N_GROUPS)
    b = np.concatenate(_groups(dt))
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def pair_set(dt, tail=False):
    """The pair set in storage type; tail=True appends TAIL_PAIRS."""
    a, b = pair_bits(dt)
    if tail:
        f = FIXED[dt]
        a = np.concatenate([a, np.array([f[i] for i, _ in TAIL_PAIRS], np.uint16)])
        b = np.concatenate([b, np.array([f[j] for _, j in TAIL_PAIRS], np.uint16)])
    return storage(dt, a), storage(dt, b)


def fold_partners(dt):
    """The fixed partners that are finite and positive, +0 among them (its negative is -0): 10 patterns.
    The input left without its negative is the largest subnormal at nb = 7 and the mid subnormal at
    nb = 15, so the subnormal results do not die out as inputs are added."""
    return [v for v in FIXED[dt] if v < INF[dt]]


@functools.lru_cache(maxsize=None)
def _fold_bits(dt, nb):
    a, b = pair_bits(dt)
    gs = _groups(dt)
    xs = [a, b, np.concatenate([gs[(g + 5) % N_GROUPS] for g in range(N_GROUPS)])]
    q = fold_partners(dt)
    for i in range(3, nb + 1):                      # x_3 = +q_0, x_4 = -q_0, x_5 = +q_1, ...
        j = (i - 3) // 2
        xs.append(np.full(N_PAIRS, q[j % len(q)] | (0x8000 if (i - 3) % 2 else 0), np.uint16))
    for x in xs:
        x.setflags(write=False)
    return xs[:nb + 1]


def fold_set(dt, nb):
    """x_0 .. x_nb (the fold's `a` and its nb received inputs) in storage type. With every further
    input drawn from the groups NaN and inf swamp the set (at nb = 15 every result is a NaN), so the
    inputs from x_3 on are constants that cancel in pairs."""
    return [storage(dt, x) for x in _fold_bits(dt, nb)]


# ---- the pack set --------------------------------------------------------------------------------
PACK_NANS = np.array([0x7f800001, 0x7f801fff, 0x7f802000, 0x7fa00000, 0xff800001, 0x7fc00000, 0xffc00001,
                      0x7fffffff, 0x7f80ffff, 0xff810000], dtype=np.uint32)


def wire_value64(dt, mag):
    """The exact values of non-negative finite wire patterns, as float64 (past max: 2^16 for fp16 and
    2^128 for bf16, the value the next pattern would have without an inf)."""
    mag = np.asarray(mag, dtype=np.int64)
    m, bias = MANT[dt], {DT_HALF: 15, DT_BFLOAT16: 127}[dt]
    e, frac = mag >> m, mag & ((1 << m) - 1)
    sub = np.ldexp(frac.astype(np.float64), 1 - bias - m)
    nor = np.ldexp((frac + (1 << m)).astype(np.float64), (e - bias - m).astype(np.int64))
    return np.where(e == 0, sub, nor)


@functools.lru_cache(maxsize=None)
def pack_set(dt):
    """fp32 inputs of the converting pack: for every finite wire pattern its exact value, the exact
    midpoint to the next pattern of larger magnitude (past max: to 2^16 for fp16 and 2^128 for bf16;
    a midpoint that is no finite fp32 would be dropped, but both last midpoints, 65520 and 0x7f7f8000,
    are finite) and the midpoint's two fp32 neighbours; then ±inf, ±the largest fp32 and PACK_NANS.
    Layout: per sign the values, the midpoints, their lower and their upper neighbours."""
    mag = np.arange(INF[dt], dtype=np.int64)
    v, nxt = wire_value64(dt, mag), wire_value64(dt, mag + 1)
    mid64 = (v + nxt) / 2                           # exact in float64: neighbours differ by one quantum
    keep = mid64 <= float(np.finfo(np.float32).max)
    with np.errstate(over='ignore'):
        mid = mid64.astype(np.float32)
    assert np.array_equal(mid[keep].astype(np.float64), mid64[keep]), 'a midpoint is not exact in fp32'
    mid = mid[keep]
    val = v.astype(np.float32)
    assert np.array_equal(val.astype(np.float64), v)
    below, above = np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf))
    pos = [val, mid, below, above]
    fmax = np.float32(np.finfo(np.float32).max)
    x = np.concatenate([p for p in pos] + [-p for p in pos] +
                       [np.array([np.inf, -np.inf, fmax, -fmax], np.float32), PACK_NANS.view(np.float32)])
    x.setflags(write=False)
    return x


def pack_midpoints(dt):
    """Boolean mask of the exact midpoints inside pack_set(dt)."""
    n = k = INF[dt]
    per_sign = n + 3 * k
    mask = np.zeros(pack_set(dt).size, bool)
    for s in range(2):
        mask[s * per_sign + n:s * per_sign + n + k] = True
    return mask


# ---- fp32 / fp64 edge table ----------------------------------------------------------------------
def edge_values(dt):
    """About 40 values: the AVG kernel test's edge set (zeros, subnormals, tiny, max, inf, NaN) plus
    ±max/2, nextafter(max, 0), 1, 1 + eps, -1 and 2^-60."""
    from test_avg_kernel_gpu import _edge_set
    T = NP[dt]
    f = np.finfo(T)
    more = np.array([f.max / 2, -f.max / 2, np.nextafter(f.max, T(0)), 1.0, T(1) + f.eps, -1.0, 2.0 ** -60], dtype=T)
    return np.concatenate([_edge_set(dt), more])


TABLE_TAIL = 2


def edge_table(dt, tail=TABLE_TAIL):
    """E x E as two arrays (a slow, b fast), and `tail` more pairs behind it (overflow, subnormal
    carry) so that the count is no multiple of the 16-byte vector."""
    E = edge_values(dt)
    a, b = np.repeat(E, E.size), np.tile(E, E.size)
    f = np.finfo(NP[dt])
    ta = np.array([f.max, f.smallest_subnormal], dtype=NP[dt])[:tail]
    tb = np.array([f.max, np.nextafter(f.tiny, NP[dt](0))], dtype=NP[dt])[:tail]
    return np.concatenate([a, ta]), np.concatenate([b, tb])


def np_add(xs):
    """Left fold of fp32 / fp64 arrays with numpy's `+`."""
    with np.errstate(all='ignore'):
        acc = xs[0].copy()
        for x in xs[1:]:
            acc = acc + x
    return acc


# ---- numpy restatement of the 16-bit arithmetic, with hooks for the mutants ---------------------
def np_fold(dt, xs, narrow_fn=None, each_add=False):
    """widen every input (exact), add left to right in fp32, narrow once (each_add: after every add)."""
    nf = narrow_fn or (lambda s: bits_of(narrow(dt, s)))
    with np.errstate(all='ignore'):
        acc = widen(dt, storage(dt, bits_of(xs[0])))
        for x in xs[1:]:
            acc = acc + widen(dt, storage(dt, bits_of(x)))
            if each_add:
                acc = widen(dt, storage(dt, nf(acc)))
    return storage(dt, nf(acc))


def is_subnormal(dt, x):
    b = bits_of(x)
    return ((b & INF[dt]) == 0) & ((b & 0x7fff) != 0)


def is_inf(dt, x):
    return (bits_of(x) & 0x7fff) == INF[dt]


def is_finite(dt, x):
    return (bits_of(x) & 0x7fff) < INF[dt]


def classes(dt, xs, out):
    """Counts of the result classes the sets are built for: subnormal results, inf from finite inputs,
    NaN results, and the NaN share."""
    finite_in = np.logical_and.reduce([is_finite(dt, x) for x in xs])
    nan = is_nan(dt, out)
    return {'subnormal': int(is_subnormal(dt, out).sum()), 'finite_to_inf': int((is_inf(dt, out) & finite_in).sum()),
            'nan': int(nan.sum()), 'nan_share': float(nan.mean())}


def bf16_ties(xs):
    """(exact ties of the fp32 sum at the bf16 rounding, those of them rounded to the even pattern
    below): the sum's low half is exactly 0x8000."""
    with np.errstate(all='ignore'):
        s = np_add([widen(DT_BFLOAT16, bits_of(x)) for x in xs]).view(np.uint32)
    tie = ((s & 0xffff) == 0x8000) & ((s & 0x7fffffff) < 0x7f800000)
    return int(tie.sum()), int((tie & ((s >> 16) & 1 == 0)).sum())


# mutants: what a subtly wrong kernel would compute
def flush_results(dt, out):
    b = bits_of(out).copy()
    sub = is_subnormal(dt, out)
    b[sub] &= 0x8000
    return storage(dt, b)


def flush_inputs(dt, x):
    return flush_results(dt, x)


def saturate(dt, xs, out):
    """inf from finite inputs becomes ±max."""
    b = bits_of(out).copy()
    hit = is_inf(dt, out) & np.logical_and.reduce([is_finite(dt, x) for x in xs])
    b[hit] -= 1
    return storage(dt, b)


def narrow_ties_away(dt, s):
    """fp32 -> wire patterns with exact ties rounded away from zero (RNE everywhere else)."""
    s = np.ascontiguousarray(s, dtype=np.float32)
    if dt == DT_BFLOAT16:
        u = s.view(np.uint32)
        r = ((u.astype(np.uint64) + 0x8000) >> 16).astype(np.uint16)
        return np.where((u & 0x7fffffff) > 0x7f800000, bits_of(narrow(dt, s)), r)
    rne = bits_of(narrow(dt, s)).copy()
    fin = np.isfinite(s) & (s != 0)
    v = np.abs(np.where(fin, s, np.float32(1)).astype(np.float64))
    _, e = np.frexp(v)
    q = np.ldexp(1.0, np.maximum(e - 1, -14) - 10)   # the fp16 quantum at v
    t = v / q                                        # exact: a power-of-two scaling
    tie = fin & (t - np.floor(t) == 0.5)
    with np.errstate(over='ignore'):
        away = ((np.floor(t) + 1) * q).astype(np.float16).view(np.uint16) | (s.view(np.uint32) >> 16 & 0x8000).astype(np.uint16)
    rne[tie] = away[tie]
    return rne


def narrow_truncate_bf16(s):
    u = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32)
    return np.where((u & 0x7fffffff) > 0x7f800000, bits_of(narrow(DT_BFLOAT16, s)), (u >> 16).astype(np.uint16))


def narrow_bf16_no_nan_test(s):
    """The integer rounding (u + 0x7fff + lsb) >> 16 applied to NaNs too."""
    u = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff).astype(np.uint16)


def count_diffs(dt, got, want):
    """How many elements assert_same's rule rejects: a NaN where none is expected or the reverse, or
    other bits where the expected value is no NaN."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    bits = {2: np.uint16, 4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
    gn, wn = is_nan(dt, got), is_nan(dt, want)
    return int(((gn != wn) | (~wn & ~gn & (got.view(bits) != want.view(bits)))).sum())


FLOAT_TYPES = [DT_FLOAT, DT_DOUBLE]
