"""The canonical order of the engine's sum of squares (include/ddl_amd.h, "Sum of squares"; the
kernels are csrc/pack.hip k_seg_sumsq and k_sumsq_finish), restated in NumPy so that the bits can
be compared. Every step is an IEEE fp64 addition of the same two numbers the kernel adds."""
import numpy as np


def _butterfly(s):
    """s[l] += s[l ^ d] for d = 32 .. 1, as lane 0 sees it: (..., 64) -> (...)."""
    d = 32
    while d >= 1:
        s = s[..., :d] + s[..., d:2 * d]
        d //= 2
    return s[..., 0]


def piece(values, compressed):
    """One piece: `values` fp32, 256 elements per tile and 4 per lane, or 512 and 8 when compressed."""
    x = np.ascontiguousarray(values, dtype=np.float32).ravel()
    n = x.size
    if n == 0:
        return 0.0
    per_lane = 8 if compressed else 4
    per_tile = 64 * per_lane
    tiles = -(-n // per_tile)
    sq = np.zeros(tiles * per_tile, np.float64)  # elements past the end count as +0.0
    xd = x.astype(np.float64)
    sq[:n] = xd * xd  # exact
    sq = sq.reshape(tiles, 64, per_lane)
    lane = np.zeros((tiles, 64), np.float64)
    for k in range(per_lane):  # left to right, from +0.0
        lane = lane + sq[:, :, k]
    v = _butterfly(lane)
    while True:  # groups of 4096 values; a piece of more than 4096 tiles takes a second level
        v = np.array([_group(v[g:g + 4096]) for g in range(0, v.size, 4096)], np.float64)
        if v.size == 1:
            return float(v[0])


def _group(v):
    """Up to 4096 values: lane l adds values l, l + 64, l + 128, ... to +0.0, then the butterfly."""
    rows = -(-v.size // 64)
    p = np.zeros(rows * 64, np.float64)
    p[:v.size] = v
    p = p.reshape(rows, 64)
    q = np.zeros(64, np.float64)
    for r in range(rows):
        q = q + p[r]
    return _butterfly(q)


def mirror(values_fp32, compressed, cuts=()):
    """The request's value: its pieces (cut at the element offsets `cuts`) added in increasing offset,
    starting from the first piece's value."""
    x = np.ascontiguousarray(values_fp32, dtype=np.float32).ravel()
    edges = [0] + sorted(int(c) for c in cuts if 0 < int(c) < x.size) + [x.size]
    total = None
    with np.errstate(all='ignore'):
        for a, b in zip(edges, edges[1:]):
            v = piece(x[a:b], compressed)
            total = v if total is None else float(np.float64(total) + np.float64(v))
    return 0.0 if total is None else total


def exact_bound(n):
    """Relative error of any summation order of n non-negative terms against the exact sum."""
    if n <= 1:
        return 0.0
    u = (n - 1) * 2.0 ** -53
    return u / (1.0 - u)
