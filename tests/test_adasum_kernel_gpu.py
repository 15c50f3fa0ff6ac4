"""The Adasum kernels (csrc/adasum.hip) through ddl_testing_thread_adasum, P virtual ranks, against the fp64 tree."""
import functools

import numpy as np
import pytest

from _adasum_helpers import LENGTHS, RANKS, max_excess, random_inputs, run_thread_adasum, tree

pytestmark = pytest.mark.gpu


@functools.lru_cache(None)
def cases(P, lengths=LENGTHS):
    """(inputs, fp64 tree per tensor): computed once, shared, never written to."""
    xs = random_inputs(P, lengths)
    return xs, [tree(col) for col in zip(*xs)]


def _same_bits(outs, want, what):
    bad = [(r, i) for r, row in enumerate(outs) for i, o in enumerate(row) if o.tobytes() != want[i].tobytes()]
    assert not bad, f'{what}: (rank, tensor) {bad}'


@pytest.mark.parametrize('P', RANKS)
def test_exact_known_answers(lib, gpu, P):
    """Bit for bit: identical tensors give that tensor (weights 2^-k, through the carry at P = 3 and 5);
    disjoint supports the plain sum; all ranks but one zero that one's tensor; all zeros zeros, not NaN."""
    base = cases(P)[0][0]
    zeros = [np.zeros_like(x) for x in base]
    _same_bits(run_thread_adasum(lib, [base] * P), base, 'identical')
    apart = [[np.where(np.arange(x.size) % P == r, x, np.float32(0)) for x in base] for r in range(P)]
    _same_bits(run_thread_adasum(lib, apart), [np.sum(col, axis=0) for col in zip(*apart)], 'disjoint')
    _same_bits(run_thread_adasum(lib, [base if r == P // 2 else zeros for r in range(P)]), base, 'one non-zero')
    _same_bits(run_thread_adasum(lib, [zeros] * P), zeros, 'all zeros')


@pytest.mark.parametrize('P,lengths', [(P, LENGTHS) for P in RANKS] + [(P, LENGTHS + (256 * 2048 + 1,)) for P in (2, 3)])
def test_random_inputs_against_the_tree(lib, gpu, P, lengths):
    """|out - ref| <= 2^-24 |ref| + FLOOR (_adasum_helpers); the same bits on every rank and in a second run;
    power-of-two factors scale exactly; a NaN in one rank's tensor k makes tensor k NaN everywhere and leaves
    k - 1 and k + 1 alone (P = 1: the input). The 257-tile tensor at P = 2, 3 takes two finish groups."""
    xs, refs = cases(P, lengths)
    outs = run_thread_adasum(lib, xs)
    assert [max_excess(o, ref) <= 0.0 for o, ref in zip(outs[0], refs)] == [True] * len(refs)
    _same_bits(outs, outs[0], 'ranks differ')
    _same_bits(run_thread_adasum(lib, xs), outs[0], 'second run')
    _same_bits(run_thread_adasum(lib, xs, post=0.5), [np.float32(0.5) * o for o in outs[0]], 'postscale 0.5')
    _same_bits(run_thread_adasum(lib, xs, pre=2.0), [np.float32(2) * o for o in outs[0]], 'prescale 2')
    bad, k = [list(row) for row in xs], 4
    bad[P - 1][k] = np.where(np.arange(LENGTHS[k]) == 17, np.float32(np.nan), xs[P - 1][k])
    for row in run_thread_adasum(lib, bad) if P > 1 else []:
        assert np.isnan(row[k]).all()
        assert all(row[i].tobytes() == outs[0][i].tobytes() for i in (k - 1, k + 1))
