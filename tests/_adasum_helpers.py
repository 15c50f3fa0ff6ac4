"""The Adasum tests' reference (include/ddl_amd.h "Adasum" as a numpy fp64 tree), inputs, bound and runner."""
import ctypes

import numpy as np

RANKS = (1, 2, 3, 4, 5, 8, 16)
LENGTHS = (1, 3, 4, 63, 64, 65, 252, 4099)  # tails, under one MFMA k-step, the 64-float slot edge, three tiles
# fp64 reassociation, Gram route against tree route, measured on the CPU by tools/adasum_floor.py on every input
# of the kernel test: 2^-48 = 3.55e-15 (at P = 8 and 16). Times 4 for the kernel's other partial-sum order.
FLOOR = 4 * 2.0 ** -48


def tree(xs, dot=lambda a, b: float(a @ b)):
    """The tree over xs in fp64 under `dot`: every level combines adjacent pairs, an odd last entry is carried up."""
    def coef(ab, nn):
        return 1.0 if nn == 0.0 else 1.0 - ab / (2.0 * nn)
    nodes = [np.asarray(x, np.float64) for x in xs]
    while len(nodes) > 1:
        pairs = [(nodes[i], nodes[i + 1], dot(nodes[i], nodes[i + 1])) for i in range(0, len(nodes) - 1, 2)]
        with np.errstate(all='ignore'):
            nodes = [coef(ab, dot(a, a)) * a + coef(ab, dot(b, b)) * b for a, b, ab in pairs] + nodes[len(pairs) * 2:]
    return nodes[0]


def random_inputs(P, lengths=LENGTHS):  # xs[r][i]: rank r's tensor i, standard normal, ranks independent
    return [[np.random.default_rng(1000 * P + 50 * r + i).standard_normal(n).astype(np.float32)
             for i, n in enumerate(lengths)] for r in range(P)]


def max_excess(out, ref):
    """max of |out - ref| - (2^-24 |ref| + FLOOR): the one fp32 rounding and the fp64 reassociation. <= 0 passes."""
    return float(np.max(np.abs(out.astype(np.float64) - ref) - 2.0 ** -24 * np.abs(ref) - FLOOR))


def run_thread_adasum(lib, xs, pre=None, post=None):
    """ddl_testing_thread_adasum over xs[r][i] (pre / post: one factor everywhere); returns outs[r][i]."""
    import torch
    P, k = len(xs), len(xs[0])
    ins = [[torch.from_numpy(x).cuda() for x in row] for row in xs]
    outs = [[torch.full_like(t, 7.0) for t in row] for row in ins]
    ptrs = [(ctypes.c_void_p * (P * k))(*[t.data_ptr() for row in ts for t in row]) for ts in (ins, outs)]
    fa = [None if f is None else (ctypes.c_float * (P * k))(*([f] * (P * k))) for f in (pre, post)]
    assert lib.ddl_testing_thread_adasum(P, k, ptrs[0], ptrs[1], (ctypes.c_size_t * k)(*[x.size for x in xs[0]]), fa[0],
                                         fa[1], torch.cuda.current_stream().cuda_stream) == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    return [[t.cpu().numpy() for t in row] for row in outs]
