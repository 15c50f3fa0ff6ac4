"""The designed inputs of test_topk_edges_gpu.py are what their names say, by the NumPy rule alone: where the threshold
lies, how many ties are taken, which tile the tie cut falls in. Conditions on the seeds, not measurements."""
import numpy as np
import pytest

from _topk_helpers import (EDGE_PPM, LANES, LONG, SUBNORMAL, TILE, count, designed, edge_inputs, keys, long_inputs,
                           nonfinite_inputs, ppm_for, reference, same_ranking_inputs, small_inputs, sparse_inputs,
                           subnormal_inputs)


def selection(a, new):
    """What the reference selected of a rank's a: the positions it zeroed (those of a non-zero a; the rest by hand)."""
    return np.flatnonzero((new.view(np.uint32) == 0) & (keys(a) != 0))


def threshold(a, ppm):
    """(T, ties, taken, the selected indices) of one rank's a, from reference()'s residual."""
    _, (new,) = reference([a], [np.zeros_like(a)], ppm)
    sel = selection(a, new)
    assert sel.size == count(a.size, ppm)  # no selected key is 0 in these families
    T = keys(a)[sel].min()
    return int(T), int((keys(a) == T).sum()), int((keys(a)[sel] == T).sum()), sel


@pytest.mark.parametrize('T', [0x3f800000, 0x3f7fffff, 0x3f8003ff, 0x3f800400, 0, 1, 0x007fffff, 0x00800000])
def test_designed_puts_the_threshold_where_it_says(T):
    n, k = 70_001, count(70_001, 10_000)
    for taken, ties in ((1, 40), (40, 40), (7, 40)) if T else ((k, n),):
        x = designed(n, k, T, ties, taken, np.random.default_rng(T % 1000 + taken))
        assert ((keys(x) > T).sum(), (keys(x) == T).sum(), (keys(x) < T).sum()) == (k - taken, ties, n - k + taken - ties)
        assert keys(x).max() <= 0x5f000000 and 0 < (x.view(np.uint32) >> 31).sum() < n
        if T:
            assert threshold(x, 10_000)[:3] == (T, ties, taken)
            assert T + 1 in keys(x) or taken == k
            assert T - 1 in keys(x)
    for bad in (dict(taken=0), dict(taken=41), dict(k=0), dict(n=700)):
        with pytest.raises(AssertionError):
            designed(**{**dict(n=n, k=k, T=T or 5, ties=40, taken=1, rng=np.random.default_rng(0)), **bad})
    with pytest.raises(AssertionError):
        designed(n, k, 0, 40, 1, np.random.default_rng(0))  # something would lie below T = 0


@pytest.mark.parametrize('last', [0, 1])
def test_edge_family(last):
    xs, plan = edge_inputs(3, last)
    for row in xs:
        for x, (T, ties, taken, n) in zip(row, plan):
            assert x.size == n and threshold(x, EDGE_PPM)[:3] == (T, ties, taken) and (taken < ties) == (not last)
    assert xs[0][0].tobytes() != xs[1][0].tobytes()


def test_sparse_family_has_a_zero_threshold():
    for P in (1, 2):
        res = None
        for step in range(2):
            xs = sparse_inputs(P, step)
            res = res or [[-np.zeros_like(x) for x in row] for row in xs]  # -0.0: a = g, the sign of a zero included
            for q in range(P):
                for i, g in enumerate(xs[q]):
                    a, k = g + res[q][i], count(g.size, 200_000)
                    nz, neg = keys(a) != 0, a.view(np.uint32) == 0x80000000
                    assert 0 < nz.sum() < k < g.size and neg.sum() > g.size // 8
                    _, (new,) = reference([g], [res[q][i]], 200_000)
                    # every non-zero is sent, then the first k - nnz zeros in index order: their -0.0 become +0.0
                    cut = np.flatnonzero(~nz)[k - nz.sum() - 1]
                    sel = nz | (np.arange(g.size) <= cut)
                    assert sel.sum() == k and not new.view(np.uint32)[sel].any()
                    assert np.array_equal(new.view(np.uint32)[~sel], a.view(np.uint32)[~sel])
                    # (the second step's first zeros stand over residuals the first step zeroed: all +0.0)
                    assert (neg & ~sel).any() and (step or (neg & sel).any())
                    assert g.size < 3 * TILE or 0 < cut // TILE < (g.size - 1) // TILE  # the cut inside a later tile
                    res[q][i] = new


@pytest.mark.parametrize('kind', ['inf', 'nan'])
def test_nonfinite_family(kind):
    xs = nonfinite_inputs(3, kind)
    for i, x in enumerate(xs[0]):
        k = count(x.size, 10_000)
        T, ties, taken, sel = threshold(x, 10_000)
        assert (T, ties, taken) == ((0x7f800000, k + 5, k) if kind == 'inf' else (0x7fc00005, 1, 1))
        assert len(set(keys(x)[sel])) == (1 if kind == 'inf' else k)
        assert all(np.isfinite(row[i]).all() for row in xs[1:])


def test_subnormal_family():
    pre, tiny = np.float32(SUBNORMAL['pre']), np.float32(2.0 ** -126)
    res, seen = subnormal_inputs(2, -1), 0
    for step in range(2):
        xs = subnormal_inputs(2, step)
        for q in range(2):
            for i, g in enumerate(xs[q]):
                assert (np.abs(g) >= tiny).all() and (np.abs(g) <= np.float32(2.0 ** -120)).all()
                assert g.size < 2049 or ((keys(res[q][i]) > 0) & (keys(res[q][i]) < 0x800000)).any()
                c, a = g * pre, g * pre + res[q][i]
                for v in (c, a):  # subnormal and not flushed
                    small = (keys(v) > 0) & (keys(v) < 0x800000)
                    assert g.size < 2049 or small.sum() > g.size // 20
                    seen += int(small.sum())
                out, (res[q][i],) = reference([g], [res[q][i]], SUBNORMAL['ppm'], pre=SUBNORMAL['pre'],
                                              post=SUBNORMAL['post'])
                assert g.size < 2049 or ((keys(out) > 0) & (keys(out) < 0x800000)).any()
    assert seen


def test_small_family_yields_every_k():
    assert [count(17, ppm_for(17, k)) for k in range(1, 18)] == list(range(1, 18))
    assert [count(2049, ppm_for(2049, k)) for k in (2, 1024, 2047, 2048)] == [2, 1024, 2047, 2048]
    assert all(set(np.abs(x)) == {1.0} for row in small_inputs('ties', 17) for x in row)


def test_long_family_cuts_the_ties_inside_a_lanes_range():
    """k_topk_offsets' lane l walks tiles [l per, (l + 1) per): the last selected tie lies in a tile that is neither
    the first nor the last of its lane's range where per = 3; with per = 2 a range has no middle, and the cut lies in a
    first tile, so the second tile's allowance (0) is what the carried count decides."""
    xs = long_inputs('pm1', 2, 0)
    for q in range(2):
        for i, n in enumerate(LONG):
            ntiles = -(-n // TILE)
            per = -(-ntiles // LANES)
            T, ties, taken, sel = threshold(xs[q][i], 500_000)
            tile = int(sel[keys(xs[q][i])[sel] == T].max()) // TILE
            assert (per, T, ties) == (2 + i, 0x3f800000, n) and taken == count(n, 500_000) < ties
            assert 0 < tile < ntiles - 1 and tile % per == (1 if per == 3 else 0)
    assert (count(LONG[1], 500_000), tile, tile // 3) == (524_291, 256, 85)
    xs = long_inputs('last_digit', 1, 0)
    for i, n in enumerate(LONG):  # gt and eq mixed in the tiles, the cut away from both ends
        T, ties, taken, sel = threshold(xs[0][i], 10_000)
        key = keys(xs[0][i])
        pad = np.zeros(-(-n // TILE) * TILE - n, bool)
        gt, eq = (np.concatenate([m, pad]).reshape(-1, TILE).sum(1) for m in (key > T, key == T))
        assert 1 <= taken < ties and (gt[:-1] > 0).all() and ((gt > 0) & (eq > 0)).sum() > gt.size // 2
        assert 0 < int(sel[key[sel] == T].max()) // TILE < gt.size - 1


@pytest.mark.parametrize('P', [8, 16])
def test_same_ranking_family(P):
    xs = [row[0] for row in same_ranking_inputs(P)]
    zero = [np.zeros_like(x) for x in xs]
    sels = [threshold(x, 100_000)[3] for x in xs]
    assert all(np.array_equal(s, sels[0]) for s in sels) and sels[0].size == 410
    mags = np.abs(np.float64(xs)[:, 0] / np.float64(xs[0][0]))  # |s_r / s_0|
    assert mags.max() / mags.min() > 2.0 ** 20 and 0 < sum(x[0] * xs[0][0] < 0 for x in xs) < P
    fwd, back = reference(xs, zero, 100_000)[0], reference(xs[::-1], zero, 100_000)[0]
    assert fwd.tobytes() != back.tobytes() and np.array_equal(np.flatnonzero(fwd), sels[0])
