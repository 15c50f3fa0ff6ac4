"""CPU model of the bf16 wire's stochastic rounding (include/ddl_amd.h "Stochastic rounding"), NumPy only:
the random bits R(S, i), the rounding rule and the host mix of the stream key S. Integer arithmetic
throughout; the only cast is _wire_helpers.narrow (torch CPU's round-to-nearest-even) for NaN and inf.

    j = i >> 1;  x = fmix32(lo32(j) ^ lo32(S));  x = fmix32(x + hi32(S) + hi32(j) * 0x9e3779b9)
    R(S, i) = bits 16 (i & 1) .. + 15 of x
    w = narrow(c) for a NaN or an infinity, else the upper 16 bits of (bits(c) + R(S, i)) mod 2^32
    S = mix64(mix64(mix64(mix64(seed) ^ rank) ^ fnv1a64(key)) ^ n)

Never the engine's own output."""
import numpy as np

from _helpers import DT_BFLOAT16
from _wire_helpers import narrow, widen

WIRE_STOCHASTIC = 0x8000  # enum ddl_allreduce_wire
M32, M64 = 0xffffffff, 0xffffffffffffffff
VALUE = 1 + 2.0 ** -10                       # the constant that reads 1.0 over the plain bf16 wire for ever
SIGMA = 2.0 ** -7 * np.sqrt(7.0 / 64.0)      # of one element's rounding error at VALUE: ulp * sqrt(p (1 - p)), p = 1/8
# fixed stream keys of the statistical checks (two arbitrary ones between the extremes)
STREAMS = [0, M64, 0x0123456789abcdef, 0x9e3779b97f4a7c15]
# +-0, the smallest subnormal, the largest finite value (to +inf for every r > 0), +-inf, quiet and signalling NaNs
EDGE_BITS = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000,
                      0x7fc00000, 0xffc00001, 0x7f800001, 0x7fffffff, 0x0000ffff, 0x00010000, 0x007fffff, 0x3f80ffff],
                     dtype=np.uint32)


def fmix32(x):
    """MurmurHash3's finaliser on a uint32 array."""
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x85ebca6b)
    x ^= x >> np.uint32(13)
    x *= np.uint32(0xc2b2ae35)
    x ^= x >> np.uint32(16)
    return x


def random_bits(S, i):
    """R(S, i) for a uint64 array of element indices: uint32 values below 65536."""
    S = int(S) & M64
    i = np.asarray(i, dtype=np.uint64)
    j = i >> np.uint64(1)
    lo, hi = (j & np.uint64(M32)).astype(np.uint32), (j >> np.uint64(32)).astype(np.uint32)
    with np.errstate(over='ignore'):
        x = fmix32(lo ^ np.uint32(S & M32))
        x = fmix32(x + np.uint32(S >> 32) + hi * np.uint32(0x9e3779b9))
    return (x >> ((i & np.uint64(1)).astype(np.uint32) * np.uint32(16))) & np.uint32(0xffff)


def round_bits(u, r):
    """The rule on raw fp32 bits u (uint32) with 16-bit integers r: bf16 bits as uint16."""
    u, r = np.asarray(u, dtype=np.uint32), np.asarray(r, dtype=np.uint32)
    special = (u & np.uint32(0x7f800000)) == np.uint32(0x7f800000)
    with np.errstate(over='ignore'):
        w = ((u + r) >> np.uint32(16)).astype(np.uint16)
    if special.any():
        w = np.where(special, narrow(DT_BFLOAT16, u.view(np.float32)), w)
    return w


def sr(x, S, first=0):
    """The stochastic pack of an fp32 array whose element e is element first + e of its request."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    i = np.uint64(first) + np.arange(x.size, dtype=np.uint64)
    return round_bits(x.view(np.uint32), random_bits(S, i))


def sr_or_cast(x, S, first=0):
    """`sr` where there is a stream, the plain cast where S is None."""
    return narrow(DT_BFLOAT16, x) if S is None else sr(x, S, first)


def mix64(z):
    z = (int(z) + 0x9e3779b97f4a7c15) & M64
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def fnv1a64(key: bytes):
    h = 0xcbf29ce484222325
    for b in key:
        h = ((h ^ b) * 0x100000001b3) & M64
    return h


def stream(seed, rank, key, n):
    """The host mix: the stream key S of the n-th request of `key` (str or bytes) on `rank`."""
    key = key.encode() if isinstance(key, str) else bytes(key)
    return mix64(mix64(mix64(mix64(int(seed) & M64) ^ int(rank)) ^ fnv1a64(key)) ^ int(n))


def mean_error(S, n, value=VALUE):
    """Mean of widen(sr(value)) - value over n elements of the constant, in fp64 (every term is exact)."""
    w = widen(DT_BFLOAT16, sr(np.full(n, value, np.float32), S)).astype(np.float64)
    return float(w.mean() - np.float64(np.float32(value)))
