"""The top-k wire's reference (include/ddl_amd.h "The top-k wire" in plain numpy fp32), the thread-world runner, and
the designed inputs of test_topk_edges_gpu.py (test_topk_inputs_cpu.py shows with the reference alone that each is
what its name says)."""
import ctypes

import numpy as np

SUM, AVG = 0, 1
LENGTHS = (1, 5, 2047, 2048, 2049, 70_001)  # both sides of a tile edge, 35 tiles, k = 1 and k = n
KEY, TILE, LANES = np.uint32(0x7fffffff), 2048, 256  # csrc/topk.hip: kKeyMask, kTile, k_topk_offsets' workgroup


def count(n, ppm):
    return min(n, max(1, -(-n * ppm // 10 ** 6)))


def ppm_for(n, k):
    """A density that sends exactly k of n."""
    ppm = k * 10 ** 6 // n
    assert count(n, ppm) == k
    return ppm


def reference(gs, rs, ppm, op=SUM, pre=1.0, post=1.0):
    """One tensor: gs[q], rs[q] per rank -> (out, new residuals). np.float32 operations only, each rounded once."""
    P, n = len(gs), gs[0].size
    out, new = np.zeros(n, np.float32), []
    with np.errstate(all='ignore'):
        for g, r in zip(gs, rs):
            a = (g if pre == 1.0 else g * np.float32(pre)) + r
            key = a.view(np.uint32) & np.uint32(0x7fffffff)
            sel = np.sort(np.lexsort((np.arange(n), -key.astype(np.int64)))[:count(n, ppm)])  # (-key, index), stable
            out[sel] += a[sel]  # in rank order; indices are unique within a rank
            keep = a.copy()
            keep[sel] = 0.0
            new.append(keep)
        if op == AVG:
            out = out / np.float32(P)
        if post != 1.0:
            out = out * np.float32(post)
    return out, new


def padded(array, off=0):
    """array on the device between guard floats of 7.0 -> (the view, a function that asserts the guards are whole).
    off 1: the view starts 4 bytes behind a 16-byte boundary."""
    import torch
    n = array.size
    buf = torch.full((n + 8,), 7.0, device='cuda')
    view = buf[4 + off:4 + off + n]
    view.copy_(torch.from_numpy(array))
    assert view.data_ptr() % 16 == 4 * off

    def check():
        assert bool((buf[:4 + off] == 7.0).all()) and bool((buf[4 + off + n:] == 7.0).all()), 'a guard was overwritten'
    return view, check


def run_thread_topk(lib, xs, res, op=SUM, pre=None, post=None, offset_out=False, offset_in=False):
    """ddl_testing_thread_topk over xs[r][i] with the residuals res[r][i] (device tensors, rewritten in place);
    returns outs[r][i]. offset_out / offset_in: every output / input starts 4 bytes behind a 16-byte boundary.
    Outputs start as 7.0 and stand, like the inputs, between guards that nothing may write."""
    import torch
    P, k = len(xs), len(xs[0])
    ins = [[padded(x, int(offset_in)) for x in row] for row in xs]
    outs = [[padded(np.full(x.size, 7.0, np.float32), int(offset_out)) for x in row] for row in xs]
    ptrs = [(ctypes.c_void_p * (P * k))(*[t.data_ptr() for row in ts for t in row])
            for ts in ([[t for t, _ in row] for row in ins], [[t for t, _ in row] for row in outs], res)]
    fa = [None if f is None else (ctypes.c_float * (P * k))(*([f] * (P * k))) for f in (pre, post)]
    assert lib.ddl_testing_thread_topk(P, k, ptrs[0], ptrs[1], ptrs[2], (ctypes.c_size_t * k)(*[x.size for x in xs[0]]),
                                       fa[0], fa[1], op, torch.cuda.current_stream().cuda_stream) == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    for _, check in (p for ps in (ins, outs) for row in ps for p in row):
        check()
    return [[t.cpu().numpy() for t, _ in row] for row in outs]


# ---- designed inputs ----

# threshold keys at the edges of the select's digits (11 / 10 / 10 bits from the top): low 20 bits 0 and all ones,
# low 10 bits all ones and 0, the middle digit's last bin, and both sides of the subnormal / normal edge (top bin 0)
EDGES = (0x3f800000, 0x3f7fffff, 0x3f8003ff, 0x3f800400, 0x3f8ffc00, 0x00000001, 0x007fffff, 0x00800000)
EDGE_LENGTHS, EDGE_TIES, EDGE_PPM = (2049, 70_001), (12, 40), 10_000
LONG = (LANES * TILE + 1, 2 * LANES * TILE + 5)  # 257 and 513 tiles: k_topk_offsets' lanes walk 2 and 3 tiles each


def keys(x):
    return x.view(np.uint32) & KEY


def designed(n, k, T, ties, taken, rng, top=0x5f000000):
    """fp32[n] in random position order with random signs whose k-th largest key is T: k - taken keys in (T, top]
    (top = 2^63: no sum of 16 overflows), `ties` keys == T of which a top-k takes `taken`, the rest in [0, T).
    T + 1 and T - 1 are present and half of the others lie within 2048 of T, so the neighbouring bins of every digit
    are occupied."""
    above, below = k - taken, n - (k - taken) - ties
    assert 1 <= taken <= ties and above >= 0 and below >= 0 and T < top and (T > 0 or below == 0)
    up, down = top - T, max(T, 1)
    hi = T + 1 + np.where(rng.random(above) < 0.5, rng.integers(0, min(2048, up), above), rng.integers(0, up, above))
    lo = T - 1 - np.where(rng.random(below) < 0.5, rng.integers(0, min(2048, down), below), rng.integers(0, down, below))
    hi[:1], lo[:1] = T + 1, T - 1
    key = rng.permutation(np.concatenate([hi, lo, np.full(ties, T)])).astype(np.uint32)
    return (key | (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31))).view(np.float32)


def edge_inputs(P, last):
    """xs[r][i] over EDGES x EDGE_LENGTHS at EDGE_PPM: the first (last: the last) of the tie run is the k-th element.
    Ranks differ by seed, not by T. Also the (T, ties, taken) of every tensor."""
    plan = [(T, ties, ties if last else 1, n) for T in EDGES for n, ties in zip(EDGE_LENGTHS, EDGE_TIES)]
    return [[designed(n, count(n, EDGE_PPM), T, ties, taken, np.random.default_rng([r, i, last]))
             for i, (T, ties, taken, n) in enumerate(plan)] for r in range(P)], plan


def sparse_inputs(P, step, lengths=(2049, 70_001)):
    """About 90 % zeros, half of them -0.0; at 200 000 ppm k is above the non-zero count, so T = 0. (-0.0 + +0.0 is
    +0.0: a keeps a -0.0 of g only over a residual of -0.0, which is what an unselected -0.0 leaves, so the first step
    starts from residuals of -0.0.)"""
    xs = []
    for r in range(P):
        row = []
        for i, n in enumerate(lengths):
            rng = np.random.default_rng([step, r, i, 90])
            x, zero = rng.standard_normal(n).astype(np.float32), rng.random(n) < 0.9
            x[zero] = np.where(rng.random(n) < 0.5, np.float32(-0.0), np.float32(0.0))[zero]
            row.append(x)
        xs.append(row)
    return xs


def nonfinite_inputs(P, kind, lengths=(2049, 70_001), ppm=10_000):
    """Finite normals; rank 0 also holds k + 5 infinities, or k + 5 NaNs of payloads 0x7fc00000 + j (random signs,
    random places): T is the inf key with k of k + 5 ties taken, or the NaN key of payload 5, a single tie."""
    xs = []
    for r in range(P):
        row = []
        for i, n in enumerate(lengths):
            rng = np.random.default_rng([r, i, 77])
            x, m = rng.standard_normal(n).astype(np.float32), count(n, ppm) + 5
            if r == 0:
                bits = np.uint32(0x7f800000) + (np.uint32(0x400000) + np.arange(m, dtype=np.uint32) if kind == 'nan' else 0)
                sign = rng.integers(0, 2, m).astype(np.uint32) << np.uint32(31)
                x.view(np.uint32)[rng.choice(n, m, replace=False)] = bits | sign
            row.append(x)
        xs.append(row)
    return xs


SUBNORMAL = dict(pre=0.3, post=1.7, ppm=900_000, lengths=(5, 2049, 70_001))


def subnormal_inputs(P, step):
    """|g| log-uniform in [2^-126, 2^-120]: with the prescale 0.3 about 3 in 10 products are subnormal.
    step -1: the residuals the first step starts from, subnormal keys 1 .. 0x7fffff."""
    xs = []
    for r in range(P):
        row = []
        for i, n in enumerate(SUBNORMAL['lengths']):
            rng = np.random.default_rng([step + 1, r, i, 126])
            sign = rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31)
            if step < 0:
                row.append((rng.integers(1, 0x800000, n).astype(np.uint32) | sign).view(np.float32))
            else:
                g = np.exp2(rng.uniform(-126, -120, n)).astype(np.float32)
                row.append((g.view(np.uint32) | sign).view(np.float32))
        xs.append(row)
    return xs


def same_ranking_inputs(P, n=4099):
    """Rank r holds s_r * base: exponents of s_r spread over 2^-12 .. 2^12, mantissas in [1, 2), mixed signs. Every
    rank ranks the keys alike (the tests assert it), so the combine adds P entries into each selected cell."""
    rng = np.random.default_rng([P, n, 12])
    base = rng.standard_normal(n).astype(np.float32)
    s = np.exp2(rng.permutation(np.linspace(-12, 12, P))) * rng.uniform(1, 2, P) * np.where(np.arange(P) % 3 == 1, -1, 1)
    return [[base * np.float32(f)] for f in s]


def long_inputs(family, P, step):
    """xs[r][i] over LONG. pm1: all +-1.0; last_digit: keys equal in their top 21 bits."""
    xs = []
    for r in range(P):
        row = []
        for i, n in enumerate(LONG):
            rng = np.random.default_rng([step, r, i, 513])
            if family == 'pm1':
                row.append(rng.choice(np.float32([-1.0, 1.0]), n))
            else:
                bits = np.uint32(0x3f800000) + rng.integers(0, 1024, n).astype(np.uint32)
                row.append((bits | (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31))).view(np.float32))
        xs.append(row)
    return xs


def small_inputs(family, n, P=2):
    """One tensor of n per rank: all +-1.0 (ties) or normals."""
    rngs = [np.random.default_rng([r, n, 17]) for r in range(P)]
    return [[rng.choice(np.float32([-1.0, 1.0]), n) if family == 'ties' else rng.standard_normal(n).astype(np.float32)]
            for rng in rngs]
