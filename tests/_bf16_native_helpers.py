"""CPU model of the sum of squares and the scale factors of a NATIVE bfloat16 keyed allreduce
(include/ddl_amd.h, the "bfloat16" paragraphs of "Sum of squares" and "Scale factors"), NumPy and the
oracle only — never the engine's own output. bf16 values are kept as raw uint16, as the other helpers do.

    contribution:  a != 1: c = narrow(widen(g) (x) a);   a == 1: the bytes
    reduction:     the plan's bf16 allreduce (oracle.fold_ref_order over the plan's unpadded bytes)
    result:        y = widen(s);  AVG and P > 1: y = y (/) float32(P);  b != 1: y = y (x) b;  narrow(y)
                   — one rounding, at the end; SUM (or P == 1) with b == 1: the bytes
    statistic:     _sumsq_helpers.mirror(widen(stored), compressed=True, cuts): the 2-byte layout's order

All arithmetic is np.float32 through _scale_helpers.mul / result; the rounding is _wire_helpers.narrow.
"""
import math
import struct

import numpy as np

from _avg_helpers import assert_same as _assert_same
from _helpers import DT_BFLOAT16
from _scale_helpers import OP_AVG, OP_SUM, mul, result  # noqa: F401  (re-exported for the tests)
from _sumsq_helpers import mirror
from _wire_helpers import narrow, widen

ALL_BITS = np.arange(65536, dtype=np.uint32).astype(np.uint16)
THIRD, THREE = np.float32(1.0 / 3.0), np.float32(3.0)
# 1 among them; 1/3 is where a rounding between quotient and factor and a truncating narrow show (13 584 and
# 21 926 of the 65 536 patterns, test_bf16_native_model_cpu.py), 3 where a factor ahead of the quotient does
FACTORS = [np.float32(v) for v in (1.0, 1.0 / 3.0, 3.0, 0.5, 2.0 ** -16)]


def bits(x):
    x = np.ascontiguousarray(x)
    assert x.dtype == np.uint16
    return x


def wide(b):
    """bf16 bits as fp32 (exact)."""
    return widen(DT_BFLOAT16, bits(b))


def rne(y):
    """fp32 -> bf16 bits, round to nearest even."""
    return narrow(DT_BFLOAT16, y)


def pack(g, a):
    """What the pack puts into the fusion buffer for the bf16 tensor g with prescale a."""
    g = bits(g)
    return g.copy() if np.float32(a) == np.float32(1) else rne(mul(wide(g), a))


def unpack(s, op, P, b):
    """What the unpack stores for the reduced bf16 stream s."""
    s = bits(s)
    if not (op == OP_AVG and P > 1) and np.float32(b) == np.float32(1):
        return s.copy()
    return rne(result(wide(s), op, P, b))


def sumsq(stored, cuts=()):
    """The statistic of the stored bf16 values."""
    return mirror(wide(stored), True, cuts)


def expected(oracle, xs, plan_bytes, op, a, b):
    """One segment's stored values: xs = the ranks' bf16 tensors in rank order, plan_bytes = the plan's
    unpadded bytes (its MPI message)."""
    P = len(xs)
    cs = [pack(x, a) for x in xs]
    total = cs[0] if P == 1 else oracle.fold_ref_order(DT_BFLOAT16, cs, plan_bytes)
    return unpack(total, op, P, b)


def assert_same(got, want, what=''):
    """Bit-equal wherever the model is not a NaN; a NaN stays a NaN."""
    _assert_same(DT_BFLOAT16, bits(got), bits(want), what)


def same_double(a, b):
    return (math.isnan(a) and math.isnan(b)) or struct.pack('<d', a) == struct.pack('<d', b)


def differing(a, b):
    """How many patterns differ between two bf16 results, NaNs compared as NaNs."""
    a, b = bits(a), bits(b)
    na, nb = (a & 0x7fff) > 0x7f80, (b & 0x7fff) > 0x7f80
    return int(((na != nb) | (~na & ~nb & (a != b))).sum())


def native_input(n, seed, specials=True):
    """A seeded bf16 segment of standard normals (RNE from fp32); with `specials` the head holds ±0, ±inf, NaN,
    the largest and the smallest normal and subnormal values, and values whose product with 3 overflows."""
    x = rne(np.random.default_rng(seed).standard_normal(n).astype(np.float32))
    if specials:
        s = np.array([0x0000, 0x8000, 0x7f80, 0xff80, 0x7fc0, 0x7f7f, 0xff7f, 0x0080, 0x0001, 0x8001, 0x007f, 0x7f00,
                      0x7eff, 0x3f80, 0xc040, 0x0002], np.uint16)
        k = min(n, s.size)
        x[:k] = s[:k]
    return x


def mixed_factors(count, shift=0):
    return [FACTORS[(i + shift) % len(FACTORS)] for i in range(count)]
