"""CPU model of the scale factors of a keyed allreduce (include/ddl_amd.h "Scale factors"), NumPy only.

All arithmetic is np.float32: round to nearest even, subnormals kept, every product rounded on its
own (NumPy never fuses a multiply with an addition).

    contribution:  c = g (x) a            (a == 1: c = g, the bits untouched)
                   wire: w = narrow(c);   feedback: v = c (+) r, then _feedback_helpers.step
    result:        y = s;  AVG: y = y (/) float32(P);  b != 1: y = y (x) b

The sums themselves come from the engine's own UNSCALED entries run on NumPy-prescaled inputs.
A NaN must be a NaN where the model has one; payloads are not compared.
"""
import numpy as np

from _feedback_helpers import step as feedback_step
from _wire_helpers import narrow, widen  # noqa: F401  (re-exported for the tests)

SCALE = 0x4000  # enum ddl_allreduce_scale
OP_SUM, OP_AVG = 0, 1
# the issue's shared inputs
LENS = [5, 300, 70_001, 4099, 1, 200_000, 513, 0]
MISALIGNED = {LENS.index(4099)}  # the tensor at a 4-byte-offset (not 16-byte aligned) address
FACTORS = [np.float32(v) for v in (1.0, 0.5, 1.0 / 3.0, 3.0, 2.0 ** -16, 1.0 / 1024.0)]


def mul(x, a):
    """x (x) a in fp32; a == 1 leaves the bits (no multiply: a NaN keeps its payload)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    a = np.float32(a)
    if a == np.float32(1):
        return x.copy()
    with np.errstate(all='ignore'):
        y = x * a
    assert y.dtype == np.float32
    return y


def result(s, op, P, b):
    """What the unpack stores for the reduced (widened) stream s: quotient, then factor."""
    y = np.ascontiguousarray(s, dtype=np.float32).copy()
    if op == OP_AVG and P > 1:
        with np.errstate(all='ignore'):
            y = (y / np.float32(P)).astype(np.float32)
    return mul(y, b)


def pack_feedback(wire_dt, g, r, a):
    """The scaled feedback pack: (w, r') for gradient g, residual r, prescale a."""
    return feedback_step(wire_dt, mul(g, a), r)


def same_bits(got, want):
    """fp32 arrays equal bit for bit, except that a NaN only has to be a NaN."""
    got = np.ascontiguousarray(got, dtype=np.float32)
    want = np.ascontiguousarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool((gn == wn).all() and (got.view(np.uint32)[~gn] == want.view(np.uint32)[~wn]).all())


def special_values(factor):
    """±0, ±inf, NaN, subnormals, values whose product with `factor` overflows and values whose product
    lands in the subnormal range (where `factor` can do either)."""
    f = np.finfo(np.float32)
    a = float(np.float32(factor))
    v = [0.0, -0.0, np.inf, -np.inf, np.nan, f.smallest_subnormal, -f.smallest_subnormal,
         float(np.nextafter(f.tiny, np.float32(0))), -float(np.nextafter(f.tiny, np.float32(0))), float(f.tiny),
         float(f.max), -float(f.max), 1.0, -3.0, 65504.0, 65520.0]
    if a > 1.0:
        v += [float(f.max) / a * 1.5, -float(f.max) / a * 1.5, float(f.max) / a]  # overflow to inf, and the edge
        v += [float(f.tiny) / a * 0.37, float(f.smallest_subnormal)]              # subnormal in, subnormal out
    if a < 1.0:
        # products in the subnormal range: 0.75 tiny, -3.3 tiny a, a value just above tiny
        v += [float(f.tiny) * 0.75 / a, -float(f.tiny) * 3.3, float(f.tiny) * 1.0000001, float(f.tiny) * 0.5 / a]
    return np.array(v, dtype=np.float32)


def scale_input(n, seed, factor=1.0):
    """A seeded fp32 segment of standard normals with the special values spliced into its head."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n).astype(np.float32)
    s = special_values(factor)
    k = min(n, s.size)
    x[:k] = s[:k]
    return x


def mixed_factors(count, shift=0):
    """Factors from FACTORS, mixed per segment (1 among them)."""
    return [FACTORS[(i + shift) % len(FACTORS)] for i in range(count)]
