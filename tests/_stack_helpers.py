"""One composed CPU model of a keyed allreduce round with every per-request option on: prescale, the
16-bit wire, error feedback, SUM / AVG, postscale and the sum of squares. NumPy only, and no arithmetic
of its own: every step is a helper that already models one option,

    c        = _scale_helpers.mul(g, a)                         the prescaled contribution
    (w, r')  = _feedback_helpers.step(wire, c, r)               or narrow(wire, c) without a residual
    s        = the ranks' w summed in MPICH's order             (oracle.fold_ref_order, per plan)
    out      = _scale_helpers.result(widen(wire, s), op, P, b)  AVG's quotient, then the postscale
    sumsq    = _sumsq_helpers.mirror(out, True, cuts)           of what is stored

so the residual is kept in PRESCALED units and the statistic is of the postscaled output. The two
stages around the sum, `pack` and `unpack`, can be swapped for wrong ones: tests/test_stack_model_cpu.py
shows that the inputs below (the GPU tests' own) tell each such mutant from the model.

Expected values never come from an engine entry that has feedback, factors or the statistic on.
"""
import math

import numpy as np

from _feedback_helpers import step_or_cast
from _helpers import DT_BFLOAT16, DT_FLOAT, DT_HALF  # noqa: F401  (re-exported for the tests)
from _mp_sumsq_worker import plan_cuts
from _scale_helpers import FACTORS, OP_AVG, OP_SUM, mixed_factors, mul, result, same_bits, scale_input  # noqa: F401
from _sumsq_helpers import mirror
from _wire_helpers import widen

ROUNDS = 3


# ---- the model ---------------------------------------------------------------------------------------
def pack(wire, g, r, a):
    """One rank's contribution: (w in the wire type, r' or None). wire 0: the fp32 product itself."""
    c = mul(g, a)
    if not wire:
        assert r is None
        return c, None
    return step_or_cast(wire, c, r)


def unpack(wire, s, op, P, b, cuts, want):
    """What is stored for the reduced stream s (wire type), and its sum of squares (+0.0 unwanted)."""
    out = result(widen(wire, s) if wire else s, op, P, b)
    return out, (mirror(out, bool(wire), cuts) if want else 0.0)


def keyed_round(gs, rs, a, wire, op, P, b, cuts, reduce, want=True, pack=pack, unpack=unpack):
    """A whole keyed round of one request. gs[q]: rank q's fp32 gradient; rs: the ranks' residuals
    (rs None, or rs[q] None: that rank runs without feedback); a / b: prescale / postscale; cuts: the
    element offsets at which the request's later pieces start (for the statistic's order);
    reduce(ws): the reduced stream from the ranks' wire values. Returns (the ranks' new residuals,
    the stored fp32 result, the sum of squares)."""
    assert len(gs) == P
    packed = [pack(wire, gs[q], None if rs is None else rs[q], a) for q in range(P)]
    out, sq = unpack(wire, reduce([w for w, _ in packed]), op, P, b, cuts, want)
    return [r for _, r in packed], out, sq


def plan_pieces(elements, esize, limit):
    """Per request the pieces [(e0, e1, message)] its fusion plans cut it into, from plan_cuts:
    message = the unpadded bytes of the plan that holds the piece. Plans are `limit`-byte stretches
    of the requests' byte stream (limit a multiple of esize); that plan_cuts' cuts are those
    stretches' ends is checked here, piece by piece."""
    assert limit % esize == 0 and all(elements)
    total, begin, rows = sum(elements) * esize, 0, []
    for n, cuts in zip(elements, plan_cuts(elements, esize, limit)):
        edges, row = [0] + list(cuts) + [n], []
        for e0, e1 in zip(edges, edges[1:]):
            p = (begin + e0 * esize) // limit
            assert (begin + e1 * esize - 1) // limit == p and (e0 == 0 or (begin + e0 * esize) % limit == 0)
            row.append((e0, e1, min(limit, total - p * limit)))
        rows.append(row)
        begin += n * esize
    return rows


def fold_pieces(oracle, dt, pieces):
    """reduce() of keyed_round: every piece summed in MPICH's order for its own plan's message."""
    def reduce(ws):
        return np.concatenate([oracle.fold_ref_order(dt, [w[e0:e1] for w in ws], message)
                               for e0, e1, message in pieces])
    return reduce


def pack_by_plans(wire, g, r, a, pieces, offset=lambda e0: 4 * e0, pack=pack):
    """`pack` as the handler runs it for a request that spans plans: piece by piece, in plan order,
    each on the window of the residual that starts `offset(e0)` BYTES into it (the contract:
    the tensor's own element offset, 4 * e0). r is updated in place; returns w. With the default
    offset this is pack() of the whole tensor; the mutants pass another."""
    assert r.flags.writeable and r.flags.c_contiguous
    ws = []
    for e0, e1, _ in pieces:
        win = np.ndarray((e1 - e0,), np.float32, buffer=r, offset=offset(e0))  # (may be 2-byte aligned only)
        w, new = pack(wire, g[e0:e1], win.copy(), a)
        win[:] = new
        ws.append(w)
    return np.concatenate(ws)


def same_double(a, b):
    return (math.isnan(a) and math.isnan(b)) or np.float64(a).tobytes() == np.float64(b).tobytes()


# ---- the thread world's inputs (tests/test_stack_engine_gpu.py) ----------------------------------------
ELEMS = [5, 300, 70_001, 4099, 1, 513]
MISALIGNED = ELEMS.index(4099)  # tensor and residual at a 4-byte-only aligned address
# AVG, SUM, AVG, ...: AVG must meet a postscale that is no power of two and no small integer (the 1/3 of
# segment 0), or taking the factor ahead of the quotient changes no bit of a widened 16-bit sum
OPS = [(i + 1) % 2 for i in range(len(ELEMS))]
PRE, POST = mixed_factors(len(ELEMS), 0), mixed_factors(len(ELEMS), 2)
WANT = [1, 0, 1, 1, 0, 1]


def no_residual(r, i):
    """Which (rank, segment) pairs run without feedback (test_feedback_engine_gpu's rule)."""
    return (r + i) % 4 == 3


def _round_input(n, seed, factor, t):
    if t == 0:
        return scale_input(n, seed, factor)
    if t == 1:
        return np.roll(scale_input(n, seed, factor), n // 2)
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def thread_inputs(P, wire, t):
    """Round t's gradients [rank][segment]: round 0 carries the specials of scale_input (inf, NaN,
    products that overflow or land among the subnormals) at the segment's head, where the residuals
    are still zero; round 1 carries them again half a segment further on, where round 0 left
    residuals (what a non-finite value does to a residual shows only there); round 2 is finite."""
    def one(r, i, n):
        return _round_input(n, 7000 + 1000 * t + 101 * P + 17 * r + i + wire, PRE[i], t)
    return [[one(r, i, n) for i, n in enumerate(ELEMS)] for r in range(P)]


def thread_model(oracle, P, wire, pack=pack, unpack=unpack, cuts=None):
    """ROUNDS rounds of the thread world from zero residuals: per round (xs, outs[i], resid[r][i],
    sq[i]). One plan whose message is all the segments' wire bytes. cuts: {segment: offsets} of the
    sub-plan pieces (the statistic's order only)."""
    message = 2 * sum(ELEMS)
    resid = [[None if no_residual(r, i) else np.zeros(n, np.float32) for i, n in enumerate(ELEMS)] for r in range(P)]
    rounds = []
    for t in range(ROUNDS):
        xs = thread_inputs(P, wire, t)
        outs, sqs, new = [], [], [[None] * len(ELEMS) for _ in range(P)]
        for i, n in enumerate(ELEMS):
            rs, out, sq = keyed_round([xs[r][i] for r in range(P)], [resid[r][i] for r in range(P)], PRE[i], wire, OPS[i],
                                      P, POST[i], (cuts or {}).get(i, ()), fold_pieces(oracle, wire, [(0, n, message)]),
                                      WANT[i], pack, unpack)
            outs.append(out)
            sqs.append(sq)
            for r in range(P):
                new[r][i] = rs[r]
        resid = new
        rounds.append((xs, outs, resid, sqs))
    return rounds


# ---- the handler batch (tests/test_stack_engine_gpu.py at P = 1, tests/_mp_stack_worker.py at P = 2, 3) ----
LIMIT = 64 << 10  # fusion_threshold_bytes
# (name, elements, feedback, wire, op, prescale, postscale, sumsq): in key order the bf16 requests form one
# group — 70_001 x 2 B spans three plans — and the uncompressed one a group of its own
BATCH = [('a_000', 5, True, DT_BFLOAT16, OP_AVG, FACTORS[1], FACTORS[3], False),
         ('a_001', 300, True, DT_BFLOAT16, OP_AVG, FACTORS[0], FACTORS[2], False),
         ('a_002', 70_001, True, DT_BFLOAT16, OP_AVG, FACTORS[2], FACTORS[5], True),
         ('b_wire', 4099, False, DT_BFLOAT16, OP_SUM, FACTORS[3], FACTORS[1], False),
         ('c_none', 513, False, 0, OP_SUM, FACTORS[1], FACTORS[2], False)]
SPANNING = 2
OTHER_COUNT = 68_001  # another element count for the spanning key: still three plans, the last above 2048 bytes


def batch_elems(count=None):
    return [count if (count and i == SPANNING) else spec[1] for i, spec in enumerate(BATCH)]


def batch_inputs(P, t, count=None):
    """Round t's tensors [rank][request], seeded by rank; the specials as in thread_inputs."""
    def one(r, i, n):
        return _round_input(n, 9100 + 500 * t + 31 * r + i, BATCH[i][5], t)
    return [[one(r, i, n) for i, n in enumerate(batch_elems(count))] for r in range(P)]


def batch_pieces(count=None):
    """Per request of BATCH its plan pieces. The two groups are planned apart. Whether the plain-wire
    request shares the feedback requests' round decides nothing that is compared: the spanning request's
    cuts lie before it, and every plan either way is more than 2048 bytes (one MPICH algorithm)."""
    n = batch_elems(count)
    return plan_pieces(n[:4], 2, LIMIT) + plan_pieces(n[4:], 4, LIMIT)


def batch_zero_residuals(P, count=None):
    return [[np.zeros(n, np.float32) if BATCH[i][2] else None for i, n in enumerate(batch_elems(count))] for _ in range(P)]


def batch_round(oracle, P, xs, resid, count=None, pack_request=None, unpack=unpack):
    """One round of BATCH: (outs[i], new resid[r][i], sq[i]). pack_request(i, wire, g, r, a, pieces)
    -> (w, r') replaces the pack of request i on every rank (the handler mutants)."""
    pieces = batch_pieces(count)
    outs, sqs, new = [], [], [[None] * len(BATCH) for _ in range(P)]
    for i, (_, _, _, wire, op, a, b, want) in enumerate(BATCH):
        def pk(w_, g, r, a_, i=i):
            return pack(w_, g, r, a_) if pack_request is None else pack_request(i, w_, g, r, a_, pieces[i])
        rs, out, sq = keyed_round([xs[q][i] for q in range(P)], [resid[q][i] for q in range(P)], a, wire, op, P, b,
                                  [e0 for e0, _, _ in pieces[i][1:]], fold_pieces(oracle, wire or DT_FLOAT, pieces[i]),
                                  want, pk, unpack)
        outs.append(out)
        sqs.append(sq)
        for q in range(P):
            new[q][i] = rs[q]
    return outs, new, sqs


# ---- the data-parallel wrapper (tests/_mp_stack_worker.check_stack_wrapper) ------------------------------
PREDIVIDE, INIT_SCALE, STEPS, INF_STEP = 2.0, 1024.0, 4, 1  # (the second step overflows on the last rank)


def mlp(torch, device):
    torch.manual_seed(4321)  # the same weights on every rank
    return torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.Tanh(), torch.nn.Linear(32, 32), torch.nn.Tanh(),
                               torch.nn.Linear(32, 4)).to(device)


def shard(torch, r):
    return torch.Generator().manual_seed(55 + r)  # its own shard of the batches


def loss_of(torch, model, gen, device, inject):
    x, y = torch.randn(8, 16, generator=gen).to(device), torch.randn(8, 4, generator=gen).to(device)
    loss = torch.nn.functional.mse_loss(model(x), y)
    return loss * math.inf if inject else loss


def wrapper_round(oracle, P, grads, resid, scale, pack=pack, unpack=unpack):
    """One allreduce_gradients() of the wrapper with bf16 feedback, fused_mean, the predivide factor
    and the loss scale `scale`: grads[i][q] = rank q's raw gradient of parameter i (of the scaled
    loss), resid[q][i] in prescaled units. One plan. Returns (outs[i], new resid, grad_norm)."""
    a, b = np.float32(1.0 / PREDIVIDE), np.float32(PREDIVIDE * (1.0 / scale))
    message = 2 * sum(g[0].size for g in grads)
    outs, sqs, new = [], [], [[None] * len(grads) for _ in range(P)]
    for i, g in enumerate(grads):
        rs, out, sq = keyed_round(g, [resid[q][i] for q in range(P)], a, DT_BFLOAT16, OP_AVG, P, b, (),
                                  fold_pieces(oracle, DT_BFLOAT16, [(0, g[0].size, message)]), True, pack, unpack)
        outs.append(out)
        sqs.append(sq)
        for q in range(P):
            new[q][i] = rs[q]
    norm = math.nan if any(math.isnan(s) for s in sqs) else math.sqrt(math.fsum(sqs))
    return outs, new, norm
