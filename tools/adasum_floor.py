"""The floor of the Adasum tests' bound (tests/_adasum_helpers.FLOOR), measured on the CPU:

  python tools/adasum_floor.py

The kernels do not walk the tree on the tensors: they walk it on weight vectors over the P inputs, every dot
product a quadratic form of the Gram matrix G = X X^T (csrc/adasum.hip). In exact arithmetic the two routes
agree; in fp64 they differ by reassociation. This prints, per P, the largest |Gram route - tree route| over the
kernel tests' own inputs, both routes in numpy fp64. The tests' floor is 4 times the largest value (the factor
covers the kernels' other partial-sum order: MFMA k-order, waves, tiles, groups)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
from _adasum_helpers import LENGTHS, RANKS, random_inputs, tree  # noqa: E402


def gram_route(xs):
    X = np.stack([np.asarray(x, np.float64) for x in xs])
    G = X @ X.T
    return tree(np.eye(len(xs)), lambda u, v: float(u @ G @ v)) @ X


worst = 0.0
for P, lengths in [(P, LENGTHS) for P in RANKS] + [(P, LENGTHS + (256 * 2048 + 1,)) for P in (2, 3)]:
    d = max(float(np.abs(gram_route(col) - tree(col)).max()) for col in zip(*random_inputs(P, lengths)))
    worst = max(worst, d)
    print(f'P = {P:2d}, {len(lengths)} tensors: {d:.3e}')
print(f'largest {worst:.3e} = 2^{np.log2(worst):.1f}; floor = 4 x that')
