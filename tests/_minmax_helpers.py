"""The reference model of DDL_ALLREDUCE_OP_MIN / _MAX (include/ddl_amd.h), in numpy on integer sort
keys, and the edge sets its tests share. Never the engine's own output.

Integers: numpy's own order (signed for int32 / int64, unsigned for uint64). Floats (fp16 as
np.float16, bf16 as raw np.uint16, fp32, fp64) are compared by bits: the key of a pattern is the
pattern with its magnitude inverted below zero, read as a signed integer — numeric order with
-0 < +0, subnormals in place, +-inf at the ends. Where any input is a NaN the result is the
canonical quiet NaN; callers compare NaN results as "is a NaN" on both sides and every other
element by its bits (assert_same). No case is ever skipped; random inputs are finite."""
import numpy as np

from _avg_helpers import assert_same, is_nan  # noqa: F401  (assert_same: the comparison rule)
from _helpers import DT_BFLOAT16, DT_DOUBLE, DT_FLOAT, DT_HALF, NP, random_input

OP_SUM, OP_AVG, OP_MIN, OP_MAX = 0, 1, 3, 4
OPS = [OP_MIN, OP_MAX]
OP_NAME = {OP_MIN: 'min', OP_MAX: 'max'}
FLOAT_DTYPES = [DT_FLOAT, DT_DOUBLE, DT_HALF, DT_BFLOAT16]

# (unsigned view, signed view, exponent mask = the +inf pattern, canonical quiet NaN)
_FMT = {DT_HALF: (np.uint16, np.int16, 0x7c00, 0x7e00),
        DT_BFLOAT16: (np.uint16, np.int16, 0x7f80, 0x7fc0),
        DT_FLOAT: (np.uint32, np.int32, 0x7f800000, 0x7fc00000),
        DT_DOUBLE: (np.uint64, np.int64, 0x7ff0000000000000, 0x7ff8000000000000)}


def float_bits(dt, x):
    return np.ascontiguousarray(x).view(_FMT[dt][0])


def sort_key(dt, bits):
    """bits ^ ((bits >> (w - 1)) & 0x7f...f), as signed integers: numeric order, -0 < +0."""
    U, S, _, _ = _FMT[dt]
    w = np.dtype(U).itemsize * 8
    s = np.ascontiguousarray(bits, dtype=U).view(S)
    return s ^ ((s >> (w - 1)) & S((1 << (w - 1)) - 1))


def nan_bits(dt, bits):
    """The magnitude is above the inf pattern."""
    U, _, inf, _ = _FMT[dt]
    mag = U((1 << (np.dtype(U).itemsize * 8 - 1)) - 1)
    return (np.asarray(bits, dtype=U) & mag) > U(inf)


def model(dt, op, xs):
    """Element-wise MIN / MAX over the arrays xs (storage type NP[dt]), in the storage type."""
    assert op in OPS and len(xs) >= 1
    xs = [np.ascontiguousarray(x) for x in xs]
    if dt not in _FMT:
        f = np.maximum if op == OP_MAX else np.minimum
        out = xs[0].copy()
        for x in xs[1:]:
            out = f(out, x)
        return out
    U, _, _, qnan = _FMT[dt]
    bits = [float_bits(dt, x) for x in xs]
    best, key = bits[0].copy(), sort_key(dt, bits[0])
    nan = nan_bits(dt, bits[0])
    for b in bits[1:]:
        k = sort_key(dt, b)
        take = k > key if op == OP_MAX else k < key
        best = np.where(take, b, best)
        key = np.where(take, k, key)
        nan = nan | nan_bits(dt, b)
    return np.where(nan, U(qnan), best).astype(U).view(NP[dt])


def finite_input(dt, n, seed):
    """Seeded finite input of dtype code dt (random_input never makes a NaN or an inf)."""
    return random_input(dt, n, seed)


def edge_bits(dt):
    """+-0, +-least and +-greatest subnormal, +-least normal, +-1 and the patterns next to it, +-max,
    +-inf, a quiet, a signalling and a negative NaN (and a negative signalling one), as bit patterns."""
    U, _, inf, qnan = _FMT[dt]
    w = np.dtype(U).itemsize * 8
    sign = 1 << (w - 1)
    mant = {DT_HALF: 10, DT_BFLOAT16: 7, DT_FLOAT: 23, DT_DOUBLE: 52}[dt]
    least_normal = 1 << mant
    one = (inf >> 1) & inf  # the exponent field 0111..1, mantissa 0
    pos = [0, 1, least_normal - 1, least_normal, one - 1, one, one + 1, inf - 1, inf]
    vals = pos + [p | sign for p in pos]
    vals += [qnan, inf | 1, qnan | sign, inf | 1 | sign, qnan | 5]
    return np.array(vals, dtype=U)


def edge_pairs(dt):
    """The edge set as all ordered pairs (a slow, b fast), in the storage type."""
    e = edge_bits(dt)
    return np.repeat(e, e.size).view(NP[dt]), np.tile(e, e.size).view(NP[dt])
