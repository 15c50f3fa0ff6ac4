"""The keyed allreduce's options TOGETHER on one GPU: error feedback with prescale / postscale, SUM and
AVG, and the sum of squares in one fusion plan of every virtual rank (thread world: FusionPipe::run with
residuals, factors and the statistic all set, unpipelined and cut into sub-plans, three rounds on the
same residuals), and through the keyed handler with a feedback request that spans three fusion plans
(its residual handed on plan by plan at the tensor's own element offset), reset_error_feedback() and a
change of the element count.

Expected: tests/_stack_helpers.py — the CPU rule for every rank's wire values and residuals, the
oracle's sum of the wire values in MPICH's order for the plan's unpadded wire bytes, NumPy's quotient and
postscale, the NumPy restatement of the statistic's order. Bit for bit; a NaN must be a NaN.
tests/test_stack_model_cpu.py shows which wrong engines these inputs reject."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _stack_helpers as sh
from _helpers import DT_BFLOAT16, DT_HALF, config
from _mp_stack_worker import check_round, submit_batch
from _scale_helpers import same_bits
from _sumsq_helpers import mirror

pytestmark = pytest.mark.gpu
K = len(sh.ELEMS)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _floats(values):
    return (ctypes.c_float * len(values))(*[float(v) for v in values])


def _place(x, i, gpu):
    """x on the device; segment MISALIGNED one float into its allocation (4-byte aligned only)."""
    if i != sh.MISALIGNED:
        return torch.from_numpy(np.array(x, dtype=np.float32)).to(gpu)
    t = torch.zeros(x.size + 1, dtype=torch.float32, device=gpu)[1:]
    assert t.data_ptr() % 16 == 4
    t.copy_(torch.from_numpy(np.array(x, dtype=np.float32)))
    return t


def _ptrs(rows):
    return (ctypes.c_void_p * (len(rows) * K))(*[t.data_ptr() if t is not None else None for row in rows for t in row])


def _run(lib, P, wire, S, D, R, want=sh.WANT):
    """One call of the composed entry: (sub-plans, sums of squares [r * K + i], cuts {segment: [elements]})."""
    J, ncuts = ctypes.c_size_t(), ctypes.c_int()
    sq, cs, ce = (ctypes.c_double * (P * K))(*([-1.0] * (P * K))), (ctypes.c_size_t * 64)(), (ctypes.c_size_t * 64)()
    st = lib.ddl_testing_thread_fused_allreduce_scale(
        P, K, S, D, R, (ctypes.c_size_t * K)(*sh.ELEMS), (ctypes.c_int * K)(*sh.OPS), wire, _floats(sh.PRE),
        _floats(sh.POST), _stream(), ctypes.byref(J), (ctypes.c_ubyte * K)(*want), sq, cs, ce, 64, ctypes.byref(ncuts))
    assert st == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    assert ncuts.value <= 64
    cuts = {}
    for c in range(ncuts.value):
        cuts.setdefault(cs[c], []).append(ce[c])
    return J.value, list(sq), cuts


@pytest.fixture(scope='module')
def model(oracle):
    """(P, wire) -> the rounds' inputs, expected outputs and residuals: computed once per pair, shared by
    the unpipelined and the pipelined run, never written to."""
    cache = {}

    def get(P, wire):
        if (P, wire) not in cache:
            rounds = sh.thread_model(oracle, P, wire)
            for xs, outs, resid, _ in rounds:
                for a in [x for row in xs for x in row] + outs + [x for row in resid for x in row if x is not None]:
                    a.setflags(write=False)
            cache[P, wire] = rounds
        return cache[P, wire]
    return get


@pytest.mark.parametrize('pipeline', [0, 64 << 10], ids=['unpipelined', 'pipelined'])
@pytest.mark.parametrize('wire', [DT_HALF, DT_BFLOAT16], ids=['fp16', 'bf16'])
@pytest.mark.parametrize('P', [2, 3])
def test_thread_world_stack(lib, gpu, model, P, wire, pipeline):
    """Three rounds on the same caller-owned residuals. After every round every rank's output, every
    residual (in prescaled units; zero where the value or its wire form was not finite) and every sum of
    squares (of the postscaled output; +0.0 where not wanted) equal the model's."""
    res = [[None if sh.no_residual(r, i) else _place(np.zeros(n, np.float32), i, gpu) for i, n in enumerate(sh.ELEMS)]
           for r in range(P)]
    R = _ptrs(res)
    with config(lib, reference_order=1, tune=0, fusion_pipeline_bytes=pipeline):
        for t, (xs, want_out, want_res, _) in enumerate(model(P, wire)):
            ins = [[_place(x, i, gpu) for i, x in enumerate(row)] for row in xs]
            outs = [[_place(np.zeros(n, np.float32), i, gpu) for i, n in enumerate(sh.ELEMS)] for _ in range(P)]
            J, sq, cuts = _run(lib, P, wire, _ptrs(ins), _ptrs(outs), R)
            assert (J > 1) == bool(pipeline)
            assert set(cuts) <= {i for i in range(K) if sh.WANT[i]} and bool(cuts) == bool(pipeline), cuts
            for i in range(K):
                what = f'P={P} round {t + 1} segment {i} (op {sh.OPS[i]}, pre {sh.PRE[i]}, post {sh.POST[i]})'
                m = mirror(want_out[i], True, cuts.get(i, ())) if sh.WANT[i] else 0.0
                for r in range(P):
                    assert same_bits(outs[r][i].cpu().numpy(), want_out[i]), what + f' rank {r}'
                    if res[r][i] is not None:
                        got = res[r][i].cpu().numpy()
                        assert same_bits(got, want_res[r][i]) and not np.isnan(got).any(), what + f' residual of rank {r}'
                    v = sq[r * K + i]
                    assert sh.same_double(v, m) and (sh.WANT[i] or not math.copysign(1.0, v) < 0), (what, r, v, m)
            for r in range(P):  # the inputs are read only
                for i in range(K):
                    assert same_bits(ins[r][i].cpu().numpy(), xs[r][i])


def test_thread_world_stack_is_race_free(lib, gpu):
    """The happens-before check over a pipelined plan with residuals, factors and the statistic, in place,
    twice on the same residuals: no pair of ops is unordered."""
    P = 3
    ins = [[_place(np.ones(n, np.float32), i, gpu) for i, n in enumerate(sh.ELEMS)] for _ in range(P)]
    res = [[_place(np.zeros(n, np.float32), i, gpu) for i, n in enumerate(sh.ELEMS)] for _ in range(P)]
    S, R = _ptrs(ins), _ptrs(res)
    counts, report = (ctypes.c_longlong * 5)(), ctypes.create_string_buffer(1 << 14)
    with config(lib, reference_order=1, tune=0, fusion_pipeline_bytes=64 << 10):
        assert lib.ddl_testing_dep_trace(1) == 0
        try:
            for _ in range(2):
                J, _, _ = _run(lib, P, DT_BFLOAT16, S, S, R)
                assert J > 1
        finally:
            torch.cuda.synchronize()
            assert lib.ddl_testing_dep_trace(0) == 0
    assert lib.ddl_testing_dep_check(counts, report, len(report)) == 0, lib.ddl_last_error()
    assert counts[0] > 0 and counts[4] == 0, report.value.decode()  # (ops, conflicts, ordered, ordered_reduce, races)


# ---- the keyed handler: a feedback request that spans fusion plans ----------------------------------------
@pytest.fixture(scope='module')
def world(gpu):
    from ddl.torch.communicator import Communicator
    return Communicator.world()


def test_handler_feedback_spans_plans(world, lib, oracle):
    """A one-rank world off the shortcut: the data plane and the wire run. 64 KiB plans cut the 70_001
    element feedback request (140 KB on the wire) into three, so plans two and three take their slice of
    its residual at elem_begin fp32 elements. The handler's residuals cannot be read: rounds 2 and 3 show
    them through the outputs. Then reset_error_feedback(), and another element count under the key: both
    restart from zero — for that key alone in the second case."""
    from ddl.torch import config as cfg
    from ddl.torch.compression import reset_error_feedback
    assert world.size == 1
    P, i = 1, sh.SPANNING
    old = cfg.get('wire_feedback_epoch')
    try:
        with config(lib, one_rank_shortcut=0, fusion_threshold_bytes=sh.LIMIT, fusion_pipeline_bytes=0):
            resid = sh.batch_zero_residuals(P)
            for t in range(sh.ROUNDS):
                xs = sh.batch_inputs(P, t)
                want_outs, resid, want_sqs = sh.batch_round(oracle, P, xs, resid)
                outs, sq = submit_batch(world, 'stk1', xs[0])
                check_round(outs, sq, want_outs, want_sqs, f'round {t + 1}')
            assert math.isfinite(want_sqs[i])
            reset_error_feedback()
            xs = sh.batch_inputs(P, 3)
            want_outs, resid, want_sqs = sh.batch_round(oracle, P, xs, sh.batch_zero_residuals(P))
            outs, sq = submit_batch(world, 'stk1', xs[0])
            check_round(outs, sq, want_outs, want_sqs, 'round 4, after reset_error_feedback()')
            # another element count under the spanning key: its residual restarts, the other keys' carry on
            n = sh.OTHER_COUNT
            xs = sh.batch_inputs(P, 4, n)
            resid[0][i] = np.zeros(n, np.float32)
            want_outs, resid, want_sqs = sh.batch_round(oracle, P, xs, resid, count=n)
            outs, sq = submit_batch(world, 'stk1', xs[0])
            check_round(outs, sq, want_outs, want_sqs, 'round 5, another element count')
            # and from there the new count's residual is carried
            xs = sh.batch_inputs(P, 5, n)
            want_outs, resid, want_sqs = sh.batch_round(oracle, P, xs, resid, count=n)
            outs, sq = submit_batch(world, 'stk1', xs[0])
            check_round(outs, sq, want_outs, want_sqs, 'round 6')
    finally:
        cfg.set('wire_feedback_epoch', old)  # (restarts every residual once more: the keys above are not used again)
