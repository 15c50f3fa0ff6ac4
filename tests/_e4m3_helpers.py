"""The block-scaled e4m3 wire (DDL_ALLREDUCE_WIRE_E4M3; include/ddl_amd.h "The e4m3 wire") restated on the CPU,
bit for bit. Never the engine's own output.

Granule: 256 bytes for 252 consecutive fp32 elements of one request: bytes 0..251 one OCP e4m3fn code each,
bytes 252..255 the bits of the fp32 scale s. Elements past the request's end count as +0.0 (code 0x00).
Pack:   c = g (or g * prescale, one fp32 product); amax over the granule's FINITE |c| (0 if none); s the smallest
        power of two with amax / s <= 448, at least 2**-126; a finite element RNE_e4m3(c / s), a NaN or an
        infinity 0x7f | sign.
Fold:   x_r = code_r * s_r in fp32, y = ((x_0 + x_1) + x_2) ... in rank order, y quantized by the pack's rule; a NaN
        sum is 0x7f whatever sign the arithmetic gave it.
Unpack: code * s, AVG's quotient by float32(P), the postscale; the request's n elements.

The quantizer is torch CPU's `.to(torch.float8_e4m3fn)`, which is RNE with subnormals for |y| <= 448 (all it ever
sees here; checked against an integer restatement in test_e4m3_model_cpu.py). The decoder is a table built from
the format's definition.
"""
import numpy as np
import torch

WIRE_E4M3 = 0x20000  # enum ddl_allreduce_wire8
G = 252              # elements per granule
GRANULE = 256        # bytes per granule
OP_SUM, OP_AVG = 0, 1


def granules(n):
    return -(-int(n) // G)


def _decode_table():
    t = np.zeros(256, np.float32)
    for c in range(256):
        e, m = (c >> 3) & 15, c & 7
        if e == 15 and m == 7:
            v = np.float32(np.nan)
        elif e == 0:
            v = np.float32(m * 2.0 ** -9)
        else:
            v = np.float32((1 + m / 8.0) * 2.0 ** (e - 7))
        bits = np.float32(v).view(np.uint32) & np.uint32(0x7fffffff) | np.uint32((c & 0x80) << 24)
        t[c] = bits.view(np.float32)
    return t


DECODE = _decode_table()


def scale_of(amax):
    """The granule scale for amax (fp32 array, finite, >= 0): the smallest power of two s with amax / s <= 448,
    at least 2**-126."""
    amax = np.asarray(amax, np.float32)
    q = amax.astype(np.float64) / 448.0  # exact where it matters: a power of two exactly when amax = 448 * 2**k
    m, e = np.frexp(q)                   # q = m * 2**e, m in [0.5, 1)
    e = np.where(m == 0.5, e - 1, e)     # the smallest power of two >= q
    e = np.where(q == 0, -126, np.maximum(e, -126))
    return np.ldexp(np.float64(1.0), e.astype(np.int64)).astype(np.float32)


def rne_codes(y):
    """RNE onto e4m3fn of finite fp32 y with |y| <= 448 (torch CPU's cast)."""
    y = np.ascontiguousarray(y, np.float32)
    assert np.all(np.abs(y) <= 448)
    return torch.from_numpy(y.copy()).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def quantize(c, rne=rne_codes, finite_amax=True, scale=scale_of):
    """fp32 contributions of one request (already prescaled) -> its granules as uint8[granules * 256]. The keyword
    arguments exist for the wrong engines of test_e4m3_model_cpu.py."""
    c = np.ascontiguousarray(c, np.float32).ravel()
    ng = granules(c.size)
    x = np.zeros(ng * G, np.float32)
    x[:c.size] = c
    x = x.reshape(ng, G)
    fin = np.isfinite(x)
    with np.errstate(all='ignore'):
        mag = np.abs(x)
        amax = np.where(fin, mag, np.float32(0)).max(axis=1) if finite_amax else np.fmax.reduce(mag, axis=1)
        amax = np.where(np.isfinite(amax), amax, np.float32(3.4028235e38)).astype(np.float32)
        s = scale(amax).astype(np.float32)
        y = (np.where(fin, x, np.float32(0)) / s[:, None]).astype(np.float32)  # exact: s is a power of two
    codes = rne(y.ravel()).reshape(ng, G).copy()
    sign = (x.view(np.uint32) >> 24).astype(np.uint8) & 0x80
    codes[~fin] = 0x7f | sign[~fin]
    out = np.zeros((ng, GRANULE), np.uint8)
    out[:, :G] = codes
    out[:, G:] = s.view(np.uint8).reshape(ng, 4)
    return out.ravel()


def dequantize(wire):
    """uint8[granules * 256] -> fp32[granules * 252]: code * s, one fp32 product each."""
    w = np.ascontiguousarray(wire, np.uint8).reshape(-1, GRANULE)
    s = w[:, G:].copy().view(np.float32)
    with np.errstate(all='ignore'):
        return (DECODE[w[:, :G]] * s).astype(np.float32).ravel()


def fold(wires, **q):
    """The schedule's reduce: the ranks' granules in rank order -> the sum's granules."""
    with np.errstate(all='ignore'):
        y = dequantize(wires[0])
        for w in wires[1:]:
            y = (y + dequantize(w)).astype(np.float32)
    y[np.isnan(y)] = np.float32(np.nan)  # the sign of a NaN sum is not IEEE's to define: 0x7f
    return quantize(y, **q)


def unpack(wire, n, op=OP_SUM, P=1, postscale=1.0):
    y = dequantize(wire)[:n]
    with np.errstate(all='ignore'):
        if op == OP_AVG:
            y = (y / np.float32(P)).astype(np.float32)
        if postscale != 1.0:
            y = (y * np.float32(postscale)).astype(np.float32)
    return y


def pack(g, prescale=1.0, **q):
    g = np.ascontiguousarray(g, np.float32)
    with np.errstate(all='ignore'):
        c = (g * np.float32(prescale)).astype(np.float32) if prescale != 1.0 else g
    return quantize(c, **q)


def allreduce(xs, op=OP_SUM, prescale=1.0, postscale=1.0):
    """The contract's result for one request: xs = the ranks' fp32 inputs in rank order. P = 1 with the data
    plane running: quantized once, no fold."""
    P = len(xs)
    wires = [pack(x, prescale) for x in xs]
    total = fold(wires) if P > 1 else wires[0]
    return unpack(total, xs[0].size, op, P, postscale)


def flat_layout(lens):
    """Byte offsets of the segments' granules in the flat buffer, and its size."""
    offs, cur = [], 0
    for n in lens:
        offs.append(cur)
        cur += granules(n) * GRANULE
    return offs, cur


def subplan_cuts(lens, cap):
    """Where fusion_pipeline_bytes = cap cuts the requests of one plan (csrc/fusion_cuts.cpp cut_plan, restated for
    granules): per request the element offsets at which a new sub-plan starts. A piece fills its sub-plan up to cap."""
    cuts, flat = [[] for _ in lens], 0
    for i, n in enumerate(lens):
        off, total = 0, granules(n) * GRANULE
        while off < total:
            if flat >= cap:
                flat = 0
            take = min(total - off, cap - flat)
            if off:
                cuts[i].append(off // GRANULE * G)
            flat += take
            off += take
    return cuts


# ---- inputs shared by the GPU tests and the wrong-engine checks of the CPU test ---------------------------------
def rank_input(n, seed, rank=0, specials=True):
    """Seeded fp32 gradients whose granules differ in magnitude by up to 2**40, with (rank 0 only, so no sum ever
    sees NaNs of both signs) +-inf, +-NaN, -0.0, an fp32 subnormal, an all-zero granule and an exact 448 spliced in."""
    rng = np.random.default_rng(1000 * seed + rank)
    x = rng.standard_normal(n).astype(np.float32)
    ng = granules(n)
    mag = np.ldexp(np.float32(1), rng.integers(-20, 21, ng)).astype(np.float32)
    x *= np.repeat(mag, G)[:n]
    if n > 3 * G:
        x[2 * G:3 * G] = 0.0  # an all-zero granule on every rank
    if specials and rank == 0:
        sp = np.array([np.inf, -np.nan, 448.0, -0.0, 1e-40, -np.inf, np.nan, 3.0e38], np.float32)
        sp[1:2] = np.array([0xffc00000], np.uint32).view(np.float32)
        pos = [p for p in (1, 5, 9, 13, G + 2, G + 7, 4 * G + 1, 5 * G + 3)]
        for p, v in zip(pos, sp):
            if p < n:
                x[p] = v
    return x


def engine_inputs(P, lens, seed):
    """xs[r][i]: rank r's tensor of request i."""
    return [[rank_input(n, seed + 17 * i, r) for i, n in enumerate(lens)] for r in range(P)]


# the requests of tests/test_e4m3_engine_gpu.py's thread worlds (and of the wrong engines of the CPU test): a
# single element, one past a granule, one past a tile, and enough granules that every rank of 16 owns several
ENGINE_LENS = [1, 253, 1009, 20_011]
ENGINE_SEED = 7
ENGINE_RANKS = [2, 3, 8, 16]
