"""The composed model of tests/_stack_helpers.py on the CPU, before the GPU tests rely on it:

  * values worked by hand are pinned: the residual is kept in prescaled units, the postscale follows
    AVG's quotient, the statistic is of what is stored;
  * a subtly wrong engine would fail: each mutant below, run in NumPy on the GPU tests' own inputs,
    differs from the model in a quantity those tests compare, by round 3 at the latest — (a) and (b)
    inside every plan slice of the spanning request but the first.

  (a) the residual slice of a spanning request taken at elem_begin * 2 bytes instead of * 4
  (b) a residual never advanced for the plans after a request's first
  (c) the product taken after the residual's addition, (g + r) * a
  (d) the postscale ahead of AVG's quotient
  (e) the sum of squares taken ahead of the postscale
  (f) a residual kept, not cleared, where v or widen(w) is not finite
  (g) a residual dropped on a skipped step
"""
import math

import numpy as np
import pytest
import torch

import _stack_helpers as sh
from _feedback_helpers import step
from _helpers import DT_BFLOAT16, DT_HALF
from _scale_helpers import OP_AVG, OP_SUM, mul, result, same_bits
from _sumsq_helpers import mirror
from _wire_helpers import widen

WIRES = [DT_HALF, DT_BFLOAT16]


# ---- the mutants -------------------------------------------------------------------------------------------
def pack_c(wire, g, r, a):
    """(c): (g + r) * a."""
    if r is None or not wire:
        return sh.pack(wire, g, r, a)
    with np.errstate(all='ignore'):
        return step(wire, mul(np.ascontiguousarray(g, dtype=np.float32) + r, a), np.zeros_like(r))


def unpack_d(wire, s, op, P, b, cuts, want):
    """(d): the factor, then the quotient."""
    out = result(mul(widen(wire, s) if wire else s, b), op, P, 1.0)
    return out, (mirror(out, bool(wire), cuts) if want else 0.0)


def unpack_e(wire, s, op, P, b, cuts, want):
    """(e): the statistic of the quotient, the factor still to come."""
    sw = widen(wire, s) if wire else s
    return result(sw, op, P, b), (mirror(result(sw, op, P, 1.0), bool(wire), cuts) if want else 0.0)


def pack_f(wire, g, r, a):
    """(f): where widen(w) is not finite the old residual stays."""
    w, new = sh.pack(wire, g, r, a)
    if new is None:
        return w, new
    return w, np.where(np.isfinite(widen(wire, w)), new, r).astype(np.float32)


def _spanning(offset):
    """(a) / (b): the handler's pack of the spanning request with the residual window at offset(e0) bytes."""
    def pack_request(i, wire, g, r, a, pieces):
        if i != sh.SPANNING:
            return sh.pack(wire, g, r, a)
        r = r.copy()
        return sh.pack_by_plans(wire, g, r, a, pieces, offset), r
    return pack_request


PACK_A, PACK_B, PACK_OK = _spanning(lambda e0: 2 * e0), _spanning(lambda e0: 0), _spanning(lambda e0: 4 * e0)


# ---- pinned values ---------------------------------------------------------------------------------------
def _fold2(oracle, wire):
    return lambda ws: oracle.fold_ref_order(wire, ws, 1 << 20)


def test_pinned_bf16_constant(oracle):
    """Two ranks hold 1 + 2^-10, prescale 0.5, AVG, postscale 2 over bf16: the contribution 0.5 + 2^-11
    is an eighth of bf16's spacing at 0.5 (2^-8) above 0.5. The residual grows by 2^-11 a round, in
    PRESCALED units; at 2^-9 the value is a tie and goes to the even 0.5; the fifth round sends
    0.5 + 2^-8 and the residual turns negative. Stored: (0.5 + 0.5) / 2 * 2 = 1, once 1 + 2^-7."""
    g = [np.full(3, 1 + 2.0 ** -10, np.float32) for _ in range(2)]
    rs = [np.zeros(3, np.float32) for _ in range(2)]
    seen, resid, sqs = [], [], []
    for _ in range(8):
        rs, out, sq = sh.keyed_round(g, rs, 0.5, DT_BFLOAT16, OP_AVG, 2, 2.0, (), _fold2(oracle, DT_BFLOAT16))
        assert (out == out[0]).all() and (rs[0] == rs[0][0]).all() and rs[0].tobytes() == rs[1].tobytes()
        seen.append(float(out[0]))
        resid.append(float(rs[0][0]))
        sqs.append(sq)
    u = 2.0 ** -11
    assert seen == [1, 1, 1, 1, 1.0078125, 1, 1, 1]
    assert resid == [u, 2 * u, 3 * u, 4 * u, -3 * u, -2 * u, -u, 0.0]
    assert sqs == [3.0, 3.0, 3.0, 3.0, 3 * 1.0078125 ** 2, 3.0, 3.0, 3.0]
    # in true units (prescale 1, postscale 1) the residual would be twice that
    r1, _, _ = sh.keyed_round(g, [np.zeros(3, np.float32)] * 2, 1.0, DT_BFLOAT16, OP_AVG, 2, 1.0, (), _fold2(oracle, DT_BFLOAT16))
    assert float(r1[0][0]) == 2 * u


def test_pinned_fp16_overflow(oracle):
    """40000 on two ranks over fp16: the sum is inf; with prescale 0.5 it is 40000 exactly and the
    residuals stay zero. 40001: the contribution 20000.5 goes as 20000 (spacing 16) and 0.5 — half
    of the gradient's 1 — stays behind; the next round sends 20001 -> 20000 again and keeps 1.0."""
    fold = _fold2(oracle, DT_HALF)
    g = [np.full(1000, 40000.0, np.float32) for _ in range(2)]
    z = [np.zeros(1000, np.float32) for _ in range(2)]
    rs, out, sq = sh.keyed_round(g, z, 1.0, DT_HALF, OP_SUM, 2, 1.0, (), fold)
    assert np.isinf(out).all() and math.isinf(sq) and not rs[0].any()  # 40000 itself is an fp16 value
    rs, out, sq = sh.keyed_round(g, z, 0.5, DT_HALF, OP_SUM, 2, 1.0, (), fold)
    assert (out == 40000.0).all() and not rs[0].any() and not rs[1].any() and sq == 1000 * 40000.0 ** 2
    rs, out, sq = sh.keyed_round(g, z, 0.5, DT_HALF, OP_AVG, 2, 2.0, (), fold)
    assert (out == 40000.0).all() and sq == 1000 * 40000.0 ** 2
    g1 = [np.full(1000, 40001.0, np.float32) for _ in range(2)]
    rs, out, _ = sh.keyed_round(g1, z, 0.5, DT_HALF, OP_SUM, 2, 1.0, (), fold)
    assert (out == 40000.0).all() and (rs[0] == 0.5).all()
    rs, out, _ = sh.keyed_round(g1, rs, 0.5, DT_HALF, OP_SUM, 2, 1.0, (), fold)
    assert (out == 40000.0).all() and (rs[0] == 1.0).all()
    # without a residual: the plain cast, and the statistic of the postscaled output
    rs, out, sq = sh.keyed_round(g1, None, 0.5, DT_HALF, OP_AVG, 2, 3.0, (), fold, want=False)
    assert rs == [None, None] and (out == 60000.0).all() and sq == 0.0 and not math.copysign(1, sq) < 0


def test_plan_pieces():
    """70_001 x 2 B behind 305 elements under 64 KiB plans: three plans, cut at 32_463 and 65_231."""
    rows = sh.batch_pieces()
    assert rows[sh.SPANNING] == [(0, 32_463, 65_536), (32_463, 65_231, 65_536), (65_231, 70_001, 17_738)]
    assert rows[0] == [(0, 5, 65_536)] and rows[3] == [(0, 4099, 17_738)] and rows[4] == [(0, 513, 2052)]
    rows = sh.batch_pieces(sh.OTHER_COUNT)
    assert len(rows[sh.SPANNING]) == 3 and rows[sh.SPANNING][2][2] - 2 * 4099 > 2048


def test_pack_by_plans_is_the_pack():
    g = sh.batch_inputs(1, 1)[0][sh.SPANNING]
    r = np.random.default_rng(1).standard_normal(g.size).astype(np.float32) * np.float32(2.0 ** -9)
    w, new = sh.pack(DT_BFLOAT16, g, r, sh.BATCH[sh.SPANNING][5])
    w2, new2 = PACK_OK(sh.SPANNING, DT_BFLOAT16, g, r, sh.BATCH[sh.SPANNING][5], sh.batch_pieces()[sh.SPANNING])
    assert w.tobytes() == w2.tobytes() and new.tobytes() == new2.tobytes()


# ---- mutant rejection: the thread world ---------------------------------------------------------------------
def _differs_thread(model, mutant, P):
    """The first round (1-based) in which a compared quantity differs, with what; None if none does."""
    for t, ((_, o0, r0, s0), (_, o1, r1, s1)) in enumerate(zip(model, mutant)):
        for i in range(len(sh.ELEMS)):
            if not same_bits(o0[i], o1[i]):
                return t + 1, f'output {i}'
            if not sh.same_double(s0[i], s1[i]):
                return t + 1, f'sumsq {i}'
            for r in range(P):
                if r0[r][i] is not None and not same_bits(r0[r][i], r1[r][i]):
                    return t + 1, f'residual {r}/{i}'
    return None


@pytest.fixture(scope='module')
def thread_models(oracle):
    cache = {}

    def get(P, wire):
        if (P, wire) not in cache:
            cache[P, wire] = sh.thread_model(oracle, P, wire)
        return cache[P, wire]
    return get


@pytest.mark.parametrize('wire', WIRES, ids=['fp16', 'bf16'])
@pytest.mark.parametrize('P', [2, 3])
def test_thread_world_inputs_reject_the_mutants(oracle, thread_models, P, wire):
    model = thread_models(P, wire)
    assert _differs_thread(model, sh.thread_model(oracle, P, wire), P) is None  # (the model is deterministic)
    for name, kw in (('c', dict(pack=pack_c)), ('d', dict(unpack=unpack_d)), ('e', dict(unpack=unpack_e)),
                     ('f', dict(pack=pack_f))):
        found = _differs_thread(model, sh.thread_model(oracle, P, wire, **kw), P)
        print(f'P={P} wire={wire} mutant ({name}): {found}')
        if name == 'd' and P == 2:
            # the quotient by 2 is exact, so (s (x) b) / 2 == (s / 2) (x) b unless an intermediate overflows or
            # lands among fp32's subnormals — which a widened fp16 cannot with these factors, and no widened
            # bf16 of these inputs does. Not a mutant at P = 2: (d) is rejected by the P = 3 cases, where the
            # quotient rounds.
            assert found is None or found[0] <= 3
            continue
        assert found is not None and found[0] <= 3, name
    # the inputs hold what the rounds are for: non-finite products in rounds 1 and 2, residuals that
    # were cleared, residuals that moved, and finite statistics in round 3
    xs0 = model[0][0]
    big = sh.ELEMS.index(70_001)
    assert any((np.isfinite(x[i]) & np.isinf(mul(x[i], sh.PRE[i]))).any() for x in xs0 for i in range(len(sh.ELEMS)))
    assert all(np.isnan(model[t][1][big]).any() for t in (0, 1)) and np.isfinite(model[2][1][big]).all()
    assert all(math.isfinite(s) for s in model[2][3])
    assert model[0][2][0][big].any() and model[2][2][0][big].any()


# ---- mutant rejection: the handler batch ----------------------------------------------------------------------
def _batch_rounds(oracle, P, rounds=sh.ROUNDS, **kw):
    resid, seen = sh.batch_zero_residuals(P), []
    for t in range(rounds):
        outs, resid, sqs = sh.batch_round(oracle, P, sh.batch_inputs(P, t), resid, **kw)
        seen.append((outs, sqs))
    return seen, resid


@pytest.fixture(scope='module')
def batch_models(oracle):
    return {P: _batch_rounds(oracle, P) for P in (1, 2, 3)}


@pytest.mark.parametrize('P', [1, 2, 3])
def test_batch_inputs_reject_the_plan_mutants(oracle, batch_models, P):
    """(a), (b): seen through the outputs alone (the handler's residuals cannot be read), in every plan
    slice of the spanning request after the first, in round 2 or 3."""
    model, _ = batch_models[P]
    same, _ = _batch_rounds(oracle, P, pack_request=PACK_OK)
    for (o0, s0), (o1, s1) in zip(model, same):
        assert all(same_bits(x, y) for x, y in zip(o0, o1)) and all(sh.same_double(x, y) for x, y in zip(s0, s1))
    i = sh.SPANNING
    slices = sh.batch_pieces()[i]
    assert len(slices) == 3
    for name, pk in (('a', PACK_A), ('b', PACK_B)):
        mutant, _ = _batch_rounds(oracle, P, pack_request=pk)
        # (a wrong window already holds the first slice's fresh residuals in round 1)
        for e0, e1, _ in slices[1:]:
            bad = [t + 1 for t in range(sh.ROUNDS) if not same_bits(model[t][0][i][e0:e1], mutant[t][0][i][e0:e1])]
            print(f'P={P} mutant ({name}) slice [{e0}, {e1}): differs in rounds {bad}')
            assert bad and set(bad) & {2, 3}, (name, e0, e1)
        assert not sh.same_double(model[2][1][i], mutant[2][1][i]), name  # and the finite sumsq of round 3


@pytest.mark.parametrize('P', [1, 2, 3])
def test_batch_inputs_reject_the_kernel_mutants(oracle, batch_models, P):
    model, _ = batch_models[P]

    def differs(mutant):
        return any(not same_bits(x, y) for (o0, _), (o1, _) in zip(model, mutant) for x, y in zip(o0, o1)) or \
            any(not sh.same_double(x, y) for (_, s0), (_, s1) in zip(model, mutant) for x, y in zip(s0, s1))
    assert differs(_batch_rounds(oracle, P, pack_request=lambda i, *a: pack_c(*a[:4]))[0])
    # ((f) touches a handful of elements here and the handler's residuals cannot be read: it is rejected by the
    # thread world, which reads them, and by the wrapper's skipped step)
    assert differs(_batch_rounds(oracle, P, unpack=unpack_e)[0])
    if P == 3:  # the quotient by 2 is exact and at P = 1 there is none: (d) is the thread world's at P = 3
        assert differs(_batch_rounds(oracle, P, unpack=unpack_d)[0])


@pytest.mark.parametrize('P', [1, 2, 3])
def test_batch_restarts_are_visible(oracle, batch_models, P):
    """Round 4 after reset_error_feedback(), and round 5 with another element count under the spanning
    key: a restart from zero gives other outputs than the residuals carried on (else the GPU test
    could not tell), in every plan slice of the spanning request."""
    _, resid = batch_models[P]
    i = sh.SPANNING
    xs = sh.batch_inputs(P, 3)
    carried, _, _ = sh.batch_round(oracle, P, xs, resid)
    fresh, r4, _ = sh.batch_round(oracle, P, xs, sh.batch_zero_residuals(P))
    for e0, e1, _ in sh.batch_pieces()[i]:
        assert not same_bits(carried[i][e0:e1], fresh[i][e0:e1])
    # round 5: the spanning key restarts (another count), the other keys carry on
    n = sh.OTHER_COUNT
    xs = sh.batch_inputs(P, 4, n)
    zero = [[np.zeros(n, np.float32) if j == i else r4[q][j] for j in range(len(sh.BATCH))] for q in range(P)]
    kept = [[r4[q][j][:n] if j == i else r4[q][j] for j in range(len(sh.BATCH))] for q in range(P)]
    want, _, _ = sh.batch_round(oracle, P, xs, zero, count=n)
    wrong, _, _ = sh.batch_round(oracle, P, xs, kept, count=n)
    assert not same_bits(want[i], wrong[i]) and same_bits(want[0], wrong[0])


# ---- mutant rejection: the wrapper -------------------------------------------------------------------------------
def wrapper_trace(oracle, P, pack=sh.pack, on_skip=None):
    """The wrapper check's steps on the CPU for all ranks at once (the same MLP, seeds and batches; the
    GPU's own gradients differ from these in their last bits only): per step (outs, norm, scale)."""
    model = sh.mlp(torch, 'cpu')
    params = list(model.parameters())
    gens = [sh.shard(torch, q) for q in range(P)]
    resid = [[np.zeros(p.numel(), np.float32) for p in params] for _ in range(P)]
    scale, clean, trace = sh.INIT_SCALE, 0, []
    for t in range(sh.STEPS):
        grads = [[None] * P for _ in params]
        for q in range(P):
            model.zero_grad()
            (sh.loss_of(torch, model, gens[q], 'cpu', t == sh.INF_STEP and q == P - 1) * scale).backward()
            for j, p in enumerate(params):
                grads[j][q] = p.grad.numpy().reshape(-1).copy()
        outs, resid, norm = sh.wrapper_round(oracle, P, grads, resid, scale, pack=pack)
        trace.append((outs, norm, scale))
        if math.isfinite(norm):
            with torch.no_grad():
                for p, o in zip(params, outs):
                    p -= 0.1 * torch.from_numpy(o).view_as(p)
            clean += 1
            if clean >= 2:
                scale, clean = scale * 2, 0
        else:
            scale, clean = scale * 0.5, 0
            if on_skip:
                resid = on_skip(resid)
    return trace


@pytest.mark.parametrize('P', [2, 3])
def test_wrapper_inputs_reject_the_mutants(oracle, P):
    """(g) a residual dropped on the skipped step and (f) one kept where v was not finite show in step
    3's gradients, and so does (c): step 2's outputs are NaN or inf throughout. The skipped step is the second, the scale goes 1024, 1024,
    512, 512."""
    model = wrapper_trace(oracle, P)
    assert [s for _, _, s in model] == [1024.0, 1024.0, 512.0, 512.0]
    assert [math.isfinite(n) for _, n, _ in model] == [True, False, True, True]

    def first(mutant):
        return next((t + 1 for t, ((o0, n0, _), (o1, n1, _)) in enumerate(zip(model, mutant))
                     if not sh.same_double(n0, n1) or any(not same_bits(x, y) for x, y in zip(o0, o1))), None)
    assert first(wrapper_trace(oracle, P)) is None
    g = first(wrapper_trace(oracle, P, on_skip=lambda resid: [[np.zeros_like(r) for r in row] for row in resid]))
    f = first(wrapper_trace(oracle, P, pack=pack_f))
    c = first(wrapper_trace(oracle, P, pack=pack_c))
    print(f'P={P}: (g) step {g}, (f) step {f}, (c) step {c}')
    assert g == 3 and f == 3 and c == 3
