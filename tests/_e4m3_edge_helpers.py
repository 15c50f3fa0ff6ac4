"""Constructed inputs for the kernels of the e4m3 wire (tests/test_e4m3_edges_gpu.py runs them on the kernels,
tests/test_e4m3_edges_cpu.py keeps what they cover from decaying): every pair of codes under a set of scale gaps for
the fold, every exponent and every element slot for the pack's scale, every code under every scale for the unpack,
ties that only a residual produces for the feedback pack. Generators only: the reference is always the model of
_e4m3_helpers / _e4m3_feedback_helpers."""
import functools

import numpy as np

import _e4m3_helpers as q8

F = np.float32
G, GRANULE = q8.G, q8.GRANULE
FLT_MAX = F(3.4028235e38)
NEG_NAN = np.array([0xffc00000], np.uint32).view(F)[0]


def bits_f32(u):
    return np.asarray(u, np.uint32).view(F)


def wire_of(codes, scale_bits):
    """codes (uint8, any length; the last granule padded with code 0) under one scale dword (or one per granule)
    -> the granules' bytes."""
    codes = np.ascontiguousarray(codes, np.uint8).ravel()
    ng = q8.granules(codes.size)
    padded = np.zeros(ng * G, np.uint8)
    padded[:codes.size] = codes
    w = np.zeros((ng, GRANULE), np.uint8)
    w[:, :G] = padded.reshape(ng, G)
    w[:, G:] = np.broadcast_to(np.asarray(scale_bits, np.uint32), (ng,)).copy().view(np.uint8).reshape(ng, 4)
    return w.ravel()


# ---- A: the fold on every pair of codes -----------------------------------------------------------------------------
# (e0, d): input 0's granules carry the scale bits e0 << 23, input 1's (e0 + d) << 23
_GAPS = [0] + [s * g for g in (1, 2, 3, 4, 5, 8, 9, 13, 21, 25) for s in (1, -1)]
PAIR_CASES = ([(127, d) for d in _GAPS]  # 21: ordinary sums, the smaller input from equal down to below half an ulp
              + [(1, d) for d in (0, 1, 4)]  # the sums are fp32 subnormals
              + [(247, d) for d in (0, 1, -1, 4, -4)])  # the sums overflow
ARRANGEMENTS = ('natural', 'shuffled', 'sorted')
PAIRS = 1 << 16
PAIR_GRANULES = q8.granules(PAIRS)  # 261
ORDER_GAPS = (-13, -21, -25)  # the order-of-addition cases: B's scale against A's


def pair_sums(e0, d):
    """The fp32 sums code0 * s0 + code1 * s1 of the 65 536 pairs in the natural order, and the exact fp64 ones."""
    k = np.arange(PAIRS)
    s0, s1 = bits_f32(e0 << 23), bits_f32((e0 + d) << 23)
    with np.errstate(all='ignore'):
        x0, x1 = (q8.DECODE[k >> 8] * s0).astype(F), (q8.DECODE[k & 255] * s1).astype(F)
        return (x0 + x1).astype(F), x0.astype(np.float64) + x1.astype(np.float64)


@functools.lru_cache(maxsize=None)
def _pair_order(e0, d, how):
    if how == 'natural':
        return np.arange(PAIRS)
    if how == 'shuffled':
        return np.random.default_rng(20_000 + 100 * e0 + d).permutation(PAIRS)
    assert how == 'sorted'
    mag = np.abs(pair_sums(e0, d)[0]).astype(np.float64)
    mag[np.isnan(mag)] = 0.0  # a NaN counts as 0; the infinities sort last by themselves
    return np.argsort(mag, kind='stable')


def pair_wires(e0, d, how='natural'):
    """[input 0, input 1]: element k of input 0 has the code order[k] >> 8, of input 1 order[k] & 255."""
    order = _pair_order(e0, d, how)
    return [wire_of((order >> 8).astype(np.uint8), e0 << 23), wire_of((order & 255).astype(np.uint8), (e0 + d) << 23)]


def order_inputs(d):
    """(B, A, C) of the order-of-addition case: A the input-0 wire at e0 = 127, B the input-1 wire d binades away,
    C = A with every code's sign flipped (-A exactly). ((B + A) + C) is B's rounding remainder against A; any order
    that adds A and C first gives B itself."""
    a, b = pair_wires(127, d)
    c = a.reshape(-1, GRANULE).copy()
    c[:, :G] ^= 0x80
    return [b, a, c.ravel()]


# ---- B: every k_foldq instantiation ----------------------------------------------------------------------------------
def crafted_inputs(nin, ng, seed):
    """test_e4m3_kernel_gpu._crafted_inputs at 29 granules (packed gradients and the crafted granules 3..8), rotated
    so that the crafted ones come first, cut to ng granules."""
    from test_e4m3_kernel_gpu import _crafted_inputs
    if ng == 29:
        return _crafted_inputs(nin, 29, seed)
    pick = (np.arange(ng) + 3) % 29
    return [w.reshape(29, GRANULE)[pick].ravel().copy() for w in _crafted_inputs(nin, 29, seed)]


BATCH_GRANULES = [29, 1, 0, 8, 9, 64, 7, 3]  # kMaxFoldBatch tables; 64 granules: 8 tiles, the others return early


def batch_inputs(nin, seed):
    """Per table of BATCH_GRANULES its nin inputs: crafted granules where they fit, packed gradients else."""
    out = []
    for i, ng in enumerate(BATCH_GRANULES):
        if ng <= 29:
            out.append(crafted_inputs(nin, ng, seed + i) if ng else [np.zeros(0, np.uint8)] * nin)
        else:
            out.append([q8.pack(q8.rank_input(ng * G - 5, seed + i, r)) for r in range(nin)])
    return out


# ---- ties of the format under a scale (C, E) -----------------------------------------------------------------------
def tie_values(s):
    """For every pair of adjacent e4m3 codes: the midpoint and its two fp32 neighbours, both signs, times the power of
    two s (exact), up to the anchor (at s = 2**120: 240 s, see anchor_of), then +-0."""
    d = q8.DECODE[:0x7f].astype(np.float64)
    mid = (d[:-1] + d[1:]) / 2 * float(s)  # exact: one more bit than a code
    mid = mid[mid <= float(anchor_of(s))]
    v = mid.astype(F)
    assert np.array_equal(v.astype(np.float64), mid)
    with np.errstate(over='ignore'):
        vals = np.concatenate([np.nextafter(v, F(0)), v, np.nextafter(v, F(np.inf))])
    vals = vals[np.isfinite(vals) & (vals <= anchor_of(s))]
    return np.concatenate([vals, -vals, np.array([0.0, -0.0], F)])


def anchor_of(s):
    """The value that pins a granule's scale to s: 448 s. At s = 2**120, the largest scale there is, 448 s is not an
    fp32 and the codes from 256 on decode to +inf (256 * 2**120 = 2**128), which is where a value above 248 * 2**120
    goes — FLT_MAX too: there the anchor is 240 s, the largest code value that is finite (its granule's scale is
    still s: 240 s / (s / 2) > 448)."""
    return F(448.0 * float(s)) if 448.0 * float(s) < float(FLT_MAX) else F(240.0 * float(s))


def sweep_values(s):
    """test_e4m3_kernel_gpu._sweep_values (an anchor that pins the granule's scale to s, then 251 values, ..., NaN,
    +-inf and -0 at the end) for every scale up to 2**120, where 448 s is not finite: the anchor is 240 s there and
    the ties past it are left out. Equal to _sweep_values(s) wherever that is defined (test_e4m3_edges_cpu.py)."""
    t = tie_values(s)[:-2]
    vals = np.concatenate([t, np.array([np.nan, np.inf, -np.inf, -0.0], F), np.array([NEG_NAN])])
    out = []
    for i in range(0, vals.size, 251):
        out.append(anchor_of(s))
        out.extend(vals[i:i + 251])
    return np.array(out, F)


# ---- C: the pack's scale at every exponent and every slot ----------------------------------------------------------
EXPONENT_MANTISSAS = (0, 0x5fffff, 0x600000, 0x600001, 0x7fffff)  # 0x600000: 1.75, the last mantissa of a scale


def exponent_maxima():
    u = np.array([(e << 23) | m for e in range(1, 255) for m in EXPONENT_MANTISSAS], np.uint32)
    u = u[u <= FLT_MAX.view(np.uint32)]
    return np.concatenate([u, np.array([0, 0x00000001, 0x007fffff], np.uint32)]).view(F)


@functools.lru_cache(maxsize=None)
def exponent_granules():
    """One granule per maximum of exponent_maxima(): the maximum at element (granule index) % 252 with alternating
    sign, the other 251 elements the ties of the scale the model assigns, those below the maximum only (where there
    are none: +-0). fp32[granules, 252]."""
    mx = exponent_maxima()
    out = np.zeros((mx.size, G), F)
    for g, m in enumerate(mx):
        t = tie_values(q8.scale_of(m))
        t = t[np.abs(t) < m]
        if t.size == 0:
            t = np.array([0.0, -0.0], F)
        row = np.resize(np.roll(t, -37 * g), G)
        row[g % G] = -m if g % 2 else m
        out[g] = row
    return out


def slot_granules(specials):
    """Granule p holds 448 * 2**(p % 40 - 20) at element p (alternating sign) and +-2**-140 everywhere else; with
    `specials` a NaN behind and an infinity ahead of it, which the amax must not see."""
    p = np.arange(G)
    x = np.full((G, G), F(2.0 ** -140), F)
    x[:, 1::2] *= F(-1)
    big = np.ldexp(F(448), p % 40 - 20).astype(F) * np.where(p % 2, F(-1), F(1))
    x[p, p] = big
    if specials:
        x[p, (p + 1) % G] = np.where(p % 3 == 0, NEG_NAN, F(np.nan))
        x[p, (p - 1) % G] = np.where(p % 2, F(np.inf), F(-np.inf))
    return x, big


# ---- D: the unpack under every scale ---------------------------------------------------------------------------------
SCALE_DWORDS = [e << 23 for e in range(256)] + [0x3fc00000, 0xbf800000, 0x7fc00000, 0x00000001, 0x007fffff]


def unpack_wire():
    """Two granules per dword of SCALE_DWORDS holding all 256 codes between them (252 + 4, the rest code 0)."""
    sc = np.repeat(np.array(SCALE_DWORDS, np.uint32), 2)
    w = wire_of(np.zeros(sc.size * G, np.uint8), sc).reshape(-1, GRANULE)
    w[0::2, :G] = np.arange(G, dtype=np.uint8)
    w[1::2, :4] = np.arange(G, 256, dtype=np.uint8)
    return w.ravel()


def unpack_segments():
    """(granules, elements) of the segments the GPU test unpacks: the whole wire in four runs of granules, the last
    one ending inside its last granule (behind the codes 252..255), then, for the sum of squares, the codes 0..126
    (no NaN code) of a few scales whose products are finite: a segment that ends inside a granule, too."""
    w = unpack_wire().reshape(-1, GRANULE)
    ng = w.shape[0]
    cuts = [0, 129, 130, 401, ng]  # odd and even starts, a single granule
    segs = [(w[a:b].ravel(), (b - a) * G) for a, b in zip(cuts, cuts[1:])]
    segs[-1] = (segs[-1][0], segs[-1][1] - (G - 4))
    for dword in (0, 1 << 23, 2 << 23, 127 << 23, 200 << 23, 246 << 23, 0x3fc00000, 0xbf800000, 0x00000001, 0x007fffff):
        g = 2 * SCALE_DWORDS.index(dword)
        segs.append((w[g].copy(), 127))
    return segs


# ---- E: the feedback pack at the edges -------------------------------------------------------------------------------
FB_SCALE_EXPONENTS = (-126, 0, 100, 120)


def _granules_behind_anchor(x, r, s):
    """251 (value, residual) pairs to a granule behind the anchor that pins the scale to s (its residual 0)."""
    xs, rs = [], []
    for i in range(0, x.size, 251):
        xs.append(anchor_of(s))
        rs.append(F(0))
        xs.extend(x[i:i + 251])
        rs.extend(r[i:i + 251])
    return np.array(xs, F), np.array(rs, F)


def fb_tie_case(s):
    """The code values themselves (both signs, up to the anchor) with residuals of half a code spacing towards either
    neighbour: every v = x + r is a tie that only the residual produced (exact: a midpoint has one more bit than a
    code). Behind them, where 448 s is finite, one granule whose largest element is exactly 448 s with a residual of
    +1 ulp of it: v is past 448 s and the scale doubles (at 2**120 there is no larger scale: left out)."""
    d = q8.DECODE[:0x7f].astype(np.float64) * float(s)
    d = d[d <= float(anchor_of(s))]
    up, down = (d[1:] - d[:-1]) / 2, -(d[1:] - d[:-1]) / 2
    x = np.concatenate([d[:-1], d[1:]])  # code c towards c + 1, code c + 1 towards c
    r = np.concatenate([up, down])
    x, r = np.concatenate([x, -x]), np.concatenate([r, -r])
    assert np.array_equal(x.astype(F).astype(np.float64), x) and np.array_equal(r.astype(F).astype(np.float64), r)
    xs, rs = _granules_behind_anchor(x.astype(F), r.astype(F), s)
    pad = -xs.size % G  # whole granules ahead of the boundary granule
    xs, rs = np.concatenate([xs, np.zeros(pad, F)]), np.concatenate([rs, np.zeros(pad, F)])
    if 448.0 * float(s) < float(FLT_MAX):
        top = F(448.0 * float(s))
        t = tie_values(s)[:200]
        bx = np.concatenate([t[:77], [top], t[77:]]).astype(F)
        br = np.zeros(bx.size, F)
        br[77] = np.nextafter(top, F(np.inf)) - top
        xs, rs = np.concatenate([xs, bx]), np.concatenate([rs, br])
    return xs, rs


def fb_overflow_case(s):
    """x = FLT_MAX with the residual FLT_MAX in the middle of a granule of ties under the scale s: v is +inf."""
    t = tie_values(s)
    xs, rs = _granules_behind_anchor(t[:400], np.zeros(400, F), s)
    xs[100], rs[100] = FLT_MAX, FLT_MAX
    return xs, rs
