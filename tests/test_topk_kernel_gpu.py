"""The top-k wire's kernels (csrc/topk.hip) through ddl_testing_thread_topk, P virtual ranks, two consecutive steps,
against the numpy rule of _topk_helpers: outputs AND residuals bit for bit."""
import numpy as np
import pytest

from _helpers import config
from _topk_helpers import AVG, LENGTHS, SUM, reference, run_thread_topk

pytestmark = pytest.mark.gpu
FAMILIES = ('normal', 'ties', 'last_digit', 'special', 'scaled', 'offset')


def inputs(family, P, step):
    """xs[r][i]. ties: all +-1.0, the index order across tiles decides; last_digit: keys equal in their top 21 bits;
    special: a NaN, an inf and -0.0 (the non-finite ones on rank 0 alone: an invalid operation's NaN sign is the CPU's)."""
    xs = []
    for r in range(P):
        row = []
        for i, n in enumerate(LENGTHS):
            rng = np.random.default_rng(10000 * step + 1000 * P + 50 * r + i)
            x = rng.standard_normal(n).astype(np.float32)
            if family == 'ties':
                x = rng.choice(np.float32([-1.0, 1.0]), n)
            elif family == 'last_digit':
                bits = np.uint32(0x3f800000) + rng.integers(0, 1024, n).astype(np.uint32)
                x = (bits | (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31))).view(np.float32)
            elif family == 'special':
                if r == 0:
                    x[0], x[n // 2] = np.nan, np.inf
                x[-1] = -0.0
            row.append(x)
        xs.append(row)
    return xs


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('op', [SUM, AVG])
@pytest.mark.parametrize('ppm', [1, 10_000, 1_000_000])
@pytest.mark.parametrize('P', [1, 2, 3, 8])
def test_two_steps_against_the_rule(lib, gpu, P, ppm, op, family):
    import torch
    pre, post = (0.3, 1.7) if family == 'scaled' else (None, None)
    res = [[torch.zeros(n, device='cuda') for n in LENGTHS] for _ in range(P)]
    ref_res = [[np.zeros(n, np.float32) for n in LENGTHS] for _ in range(P)]
    with config(lib, wire_topk_ppm=ppm):
        for step in range(2):
            xs = inputs(family, P, step)
            outs = run_thread_topk(lib, xs, res, op, pre, post, offset_out=family == 'offset')
            for i in range(len(LENGTHS)):
                want, new = reference([xs[q][i] for q in range(P)], [ref_res[q][i] for q in range(P)], ppm, op,
                                      pre or 1.0, post or 1.0)
                for q in range(P):
                    ref_res[q][i] = new[q]
                    assert outs[q][i].tobytes() == want.tobytes(), (step, q, LENGTHS[i], 'out')
                    assert res[q][i].cpu().numpy().tobytes() == new[q].tobytes(), (step, q, LENGTHS[i], 'residual')
                if ppm == 1_000_000 and pre is None:  # everything is sent: the plain rank-order fp32 sum, nothing kept
                    plain = np.zeros(LENGTHS[i], np.float32)
                    for q in range(P):
                        plain = plain + xs[q][i]
                    plain = plain / np.float32(P) if op == AVG else plain
                    assert want.tobytes() == plain.tobytes() and not any(r.view(np.uint32).any() for r in new)
