"""The top-k wire's select and emit (csrc/topk.hip) where its counting can be off by one: thresholds at the edges of the
radix digits, T = 0, inf and NaN keys, subnormal sums, every k of a small tensor, tie cuts inside a lane's run of
tiles (more than 256 tiles per tensor), everything off alignment, and P ranks sending the same indices. Outputs AND
residuals bit for bit against the numpy rule of _topk_helpers, through ddl_testing_thread_topk; test_topk_inputs_cpu.py
shows that each input is what its name says."""
import numpy as np
import pytest

from _helpers import config
from _topk_helpers import (EDGE_PPM, LENGTHS, SUBNORMAL, SUM, count, edge_inputs, keys, long_inputs, nonfinite_inputs,
                           padded, ppm_for, reference, run_thread_topk, same_ranking_inputs, small_inputs, sparse_inputs,
                           subnormal_inputs)

pytestmark = pytest.mark.gpu


def same(got, want, what):
    """Bit for bit; the first difference in the message."""
    g, w = got.view(np.uint32), want.view(np.uint32)
    if not np.array_equal(g, w):
        at = int(np.flatnonzero(g != w)[0])
        raise AssertionError(f'{what}: {int((g != w).sum())} of {g.size} differ, first at {at}: '
                             f'got {int(g[at]):#010x}, want {int(w[at]):#010x}')


def against_the_rule(lib, steps, ppm, res0=None, pre=None, post=None, off=0):
    """steps[s][r][i] through the kernels, the residuals carried (from res0[r][i], else zero) between guard floats:
    outputs and residuals against reference() after every step. -> per step (the kernels' outs[r][i] and residuals[r][i],
    a[r][i])."""
    P, lengths = len(steps[0]), [x.size for x in steps[0][0]]
    ref = [list(row) for row in res0] if res0 else [[np.zeros(n, np.float32) for n in lengths] for _ in range(P)]
    pads = [[padded(r, off) for r in row] for row in ref]
    res, seen = [[view for view, _ in row] for row in pads], []
    with config(lib, wire_topk_ppm=ppm):
        for s, xs in enumerate(steps):
            outs = run_thread_topk(lib, xs, res, SUM, pre, post, offset_out=bool(off), offset_in=bool(off))
            for _, check in (p for row in pads for p in row):
                check()
            got = [[t.cpu().numpy().copy() for t in row] for row in res]
            with np.errstate(all='ignore'):
                a = [[(xs[q][i] if pre is None else xs[q][i] * np.float32(pre)) + ref[q][i] for i in range(len(lengths))]
                     for q in range(P)]
            for i, n in enumerate(lengths):
                want, new = reference([xs[q][i] for q in range(P)], [ref[q][i] for q in range(P)], ppm, SUM,
                                      pre or 1.0, post or 1.0)
                for q in range(P):
                    ref[q][i] = new[q]
                    same(outs[q][i], want, f'step {s} rank {q} n {n} (tensor {i}) out')
                    same(got[q][i], new[q], f'step {s} rank {q} n {n} (tensor {i}) residual')
            seen.append((outs, got, a))
    return seen


@pytest.mark.parametrize('via', ['gradient', 'residual'])
@pytest.mark.parametrize('last', [0, 1])
@pytest.mark.parametrize('P', [1, 3])
def test_threshold_at_every_digit_edge(lib, gpu, P, last, via):
    """One plan of EDGES x EDGE_LENGTHS: the k-th key is the first (last: the last) of a run of ties at T, T - 1 and
    T + 1 present. The vector comes as g over a zero residual, or as the residual under g = +0.0: the keys are a's."""
    xs, _ = edge_inputs(P, last)
    if via == 'residual':
        against_the_rule(lib, [[[np.zeros_like(x) for x in row] for row in xs]], EDGE_PPM, res0=xs)
    else:
        against_the_rule(lib, [xs], EDGE_PPM)


@pytest.mark.parametrize('P', [1, 2])
def test_zero_threshold_sparse_gradient(lib, gpu, P):
    """T = 0 and bin 0 in all three passes: every zero is a tie, taken in ascending index. A selected -0.0 leaves +0.0,
    an unselected one stays -0.0, every non-zero element is sent."""
    steps = [sparse_inputs(P, step) for step in range(2)]
    res0 = [[-np.zeros_like(x) for x in row] for row in steps[0]]
    for (outs, new, a), xs in zip(against_the_rule(lib, steps, 200_000, res0=res0), steps):
        for q in range(P):
            for i, x in enumerate(xs[q]):
                k, nz = count(x.size, 200_000), keys(a[q][i]) != 0
                sel = nz | (np.arange(x.size) <= np.flatnonzero(~nz)[k - nz.sum() - 1])
                bits = new[q][i].view(np.uint32)
                assert sel.sum() == k and not bits[sel].any()
                neg = (a[q][i].view(np.uint32) == 0x80000000) & ~sel
                assert neg.any() and (bits[neg] == 0x80000000).all()
                assert np.array_equal(bits[~sel], a[q][i].view(np.uint32)[~sel])
                if P == 1:  # what was sent is what came out: every non-zero element, and only those
                    sent = outs[q][i].view(np.uint32)
                    assert np.array_equal(sent[nz], a[q][i].view(np.uint32)[nz]) and not sent[~nz].any()


@pytest.mark.parametrize('kind', ['inf', 'nan'])
def test_nonfinite_thresholds(lib, gpu, kind):
    """P = 3, rank 0 alone holds k + 5 infinities (T = the inf key, k of k + 5 ties taken) or k + 5 NaNs of payloads
    0x7fc00000 + j (the order among NaN keys decides: payloads 5 and up are sent). Outputs and residuals bit for bit:
    the sum 0.0 + NaN + finite + finite keeps the NaN's sign and payload on the GPU as in NumPy."""
    against_the_rule(lib, [nonfinite_inputs(3, kind)], 10_000)


def test_subnormal_accumulate(lib, gpu):
    """g x 0.3, that product + r, the combine's sum and its product with 1.7 are subnormal in many elements: fp32,
    round to nearest even, nothing flushed to zero (include/ddl_amd.h)."""
    against_the_rule(lib, [subnormal_inputs(2, step) for step in range(2)], SUBNORMAL['ppm'], res0=subnormal_inputs(2, -1),
                     pre=SUBNORMAL['pre'], post=SUBNORMAL['post'])


@pytest.mark.parametrize('family', ['ties', 'normal'])
def test_every_k_of_a_small_tensor(lib, gpu, family):
    for n, ks in ((17, range(1, 18)), (2049, (2, 1024, 2047, 2048))):
        xs = small_inputs(family, n)
        for k in ks:
            against_the_rule(lib, [xs], ppm_for(n, k))


@pytest.mark.parametrize('family,ppm', [('pm1', 500_000), ('last_digit', 10_000)])
def test_more_tiles_than_lanes(lib, gpu, family, ppm):
    """257 and 513 tiles in one plan: k_topk_offsets' lanes walk 2 and 3 tiles each and carry their counts, the second
    tensor starts at tile 257. pm1: the tie cut falls inside a lane's run; last_digit: gt and eq mixed in the tiles."""
    against_the_rule(lib, [long_inputs(family, 2, step) for step in range(2)], ppm)


def test_unaligned_everything(lib, gpu):
    """Inputs, outputs and residuals all 4 bytes behind a 16-byte boundary: load8 / store8 go element by element over
    whole tensors; nothing is written beside any of them."""
    steps = [[[np.random.default_rng([step, r, i, 4]).standard_normal(n).astype(np.float32) for i, n in enumerate(LENGTHS)]
              for r in range(2)] for step in range(2)]
    against_the_rule(lib, steps, 10_000, off=1)


@pytest.mark.parametrize('P', [8, 16])
def test_every_rank_selects_the_same_indices(lib, gpu, P):
    """Rank r holds s_r x base: every rank sends the same 410 of 4099 indices, so the combine adds P entries into each
    of those cells, in rank order: the reversed order gives other bits."""
    xs = same_ranking_inputs(P)
    zero = [[np.zeros_like(row[0])] for row in xs]
    (outs, new, _), = against_the_rule(lib, [xs], 100_000)
    sel = np.flatnonzero(keys(new[0][0]) == 0)
    assert sel.size == 410 and all(np.array_equal(np.flatnonzero(keys(row[0]) == 0), sel) for row in new)
    back, _ = reference([row[0] for row in xs[::-1]], [z[0] for z in zero], 100_000)
    assert back.tobytes() != outs[0][0].tobytes() and np.array_equal(np.flatnonzero(back), np.flatnonzero(outs[0][0]))
