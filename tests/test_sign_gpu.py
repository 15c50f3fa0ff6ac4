"""DDL_ALLREDUCE_WIRE_SIGN on the GPU. The kernels (csrc/sign.hip) through ddl_testing_thread_sign against the numpy
rule of _sign_helpers, outputs AND residuals bit for bit; the engine: the refusals, a mixed round on the keyed path,
the residual's restarts, the one-rank shortcut, and P = 2 processes over RCCL (_sign_helpers.check_sign_batch)."""
import ctypes

import numpy as np
import pytest
import torch

import _mp_gpu_worker
import _sign_helpers
from _helpers import DT_BFLOAT16, DT_DOUBLE, DT_FLOAT, DT_HALF, config
from _sign_helpers import AVG, BLOCK, LENGTHS, NAN, SUM, padded, reference, run_thread_sign
from test_multiproc_rccl_gpu import _run

pytestmark = pytest.mark.gpu
VP, SZ, INVALID, UNSUPPORTED_DTYPE, SIGN = ctypes.c_void_p, ctypes.c_size_t, 3, 4, 0x100000
# every other wire, feedback and stochastic bit, SUMSQ, and the ops MIN, MAX, ADASUM
FLAGS = (0x100, 0x200, 0x1000, 0x1100, 0x8000, 0x8200, 0x20000, 0x40000, 0x60000, 0x80000, 0x2000, 3, 4, 6)


def inputs(family, P, step):
    """xs[r][i]. special, at step 1 on rank 0 alone: a NaN in every first block, a block whose |a| sum overflows."""
    xs = [[np.random.default_rng(10000 * step + 1000 * P + 50 * r + i).standard_normal(n).astype(np.float32)
           for i, n in enumerate(LENGTHS)] for r in range(P)]
    for x in [x for row in xs for x in row] if family == 'zeros' else []:
        x[:] = np.where(x < 0, np.float32(-0.0), np.float32(0.0))
    for x in xs[0] if family == 'special' and step == 1 else []:
        x[0], x[2 * BLOCK:3 * BLOCK] = np.nan, 3e38
    return xs


@pytest.mark.parametrize('family', ['normal', 'zeros', 'scaled', 'offset', 'special'])
@pytest.mark.parametrize('op', [SUM, AVG])
@pytest.mark.parametrize('P', [1, 2, 3, 8])
def test_two_steps_of_one_plan_against_the_rule(lib, gpu, P, op, family):
    """offset: every input, output and residual 4 bytes off a 16-byte boundary."""
    (pre, post), off = (0.3, 1.7) if family == 'scaled' else (None, None), int(family == 'offset')
    res = [[padded(np.zeros(n, np.float32), off) for n in LENGTHS] for _ in range(P)]
    ref_res = [[np.zeros(n, np.float32) for n in LENGTHS] for _ in range(P)]
    for step in range(2):
        xs = inputs(family, P, step)
        outs = run_thread_sign(lib, xs, res, op, pre, post, off)
        for i, n in enumerate(LENGTHS):
            old = ref_res[0][i]
            want, new = reference([xs[q][i] for q in range(P)], [ref_res[q][i] for q in range(P)], op, pre or 1.0, post or 1.0)
            for q in range(P):
                ref_res[q][i] = new[q]
                assert outs[q][i].tobytes() == want.tobytes(), (step, q, n, 'out')
                assert res[q][i].cpu().numpy().tobytes() == new[q].tobytes(), (step, q, n, 'residual')
            if family == 'special' and step == 1:  # what the rule says of them: NaN blocks, rank 0's residual as it was
                bad = np.r_[0:min(n, BLOCK), 2 * BLOCK:min(n, 3 * BLOCK)]
                assert (want.view(np.uint32)[bad] == NAN).all() and new[0][bad].tobytes() == old[bad].tobytes()


def test_the_wire_is_exactly_compensated(lib, gpu):
    """P = 3, n = 2049, the same gradients for 8 steps: the sum of the outputs plus the final residuals is 8 x the
    sum of the gradients up to fp32 rounding. The numpy rule on the CPU (reference() in place of the kernels) leaves
    2.98e-6 with these sums in fp64; the bound is twice that."""
    gs = [np.random.default_rng(40 + q).standard_normal(2049).astype(np.float32) for q in range(3)]
    res, total = [[padded(np.zeros(2049, np.float32))] for _ in gs], np.zeros(2049, np.float64)
    for _ in range(8):
        total += run_thread_sign(lib, [[g] for g in gs], res)[0][0]
    kept = np.sum([r[0].cpu().numpy() for r in res], axis=0, dtype=np.float64)
    assert np.abs(total + kept - 8 * np.sum(gs, axis=0, dtype=np.float64)).max() <= 5.96e-6


def test_refusals(gpu, lib):
    """Before anything is registered; the communicator works afterwards."""
    from ddl.torch import cpp_backend as cb
    from ddl.torch.communicator import Communicator
    from ddl.torch.tensor_communicate import allreduce
    done, s, world = cb.DONE_FN(lambda status, user: None), torch.cuda.current_stream().cuda_stream, Communicator.world()
    d, h = torch.ones(16, device='cuda'), torch.ones(16)
    n1, keys = (SZ * 1)(16), (ctypes.c_char_p * 1)(b'refused')
    arg = cb.SumsqArg(None, None)  # what the SUMSQ bit makes of `user`
    users = (VP * 1)(ctypes.addressof(arg))
    cases = [(SIGN, dt, d, UNSUPPORTED_DTYPE) for dt in (DT_HALF, DT_BFLOAT16, DT_DOUBLE)] + [(SIGN, DT_FLOAT, h, INVALID)]
    for op, dt, t, status in cases + [(SIGN | f, DT_FLOAT, d, INVALID) for f in FLAGS]:
        p, arr, mem = t.data_ptr(), (VP * 1)(t.data_ptr()), cb.MEMORY_DEVICE if t.is_cuda else cb.MEMORY_HOST
        assert lib.ddl_allreduce_submit_mem(world.id, keys[0], p, p, 16, dt, op, mem, s, done, users[0]) == status, (op, dt)
        assert lib.ddl_allreduce_submit_batch_mem(world.id, 1, keys, arr, arr, n1, (ctypes.c_int * 1)(dt), op, mem,
                                                  s, done, users) == status and lib.ddl_last_error(), (op, dt)
    p, one, many = d.data_ptr(), (VP * 1)(d.data_ptr()), (VP * 17)(*([d.data_ptr()] * 17))
    assert [lib.ddl_allreduce(world.id, p, p, 16, DT_FLOAT, SIGN, s),
            lib.ddl_allreduce_batch(world.id, 1, one, one, n1, DT_FLOAT, SIGN, s),
            lib.ddl_allreduce_host(world.id, h.data_ptr(), h.data_ptr(), 16, DT_FLOAT, SIGN),
            lib.ddl_testing_thread_sign(17, 1, many, many, many, n1, None, None, SUM, s)] == [INVALID] * 4  # the last: 17 ranks
    assert lib.ddl_wait_all(world.id) == 0  # nothing was registered
    assert torch.equal(allreduce(d, world), d)  # a SUM still works


def test_a_mixed_round_and_the_residuals_restarts(gpu, lib):
    """P = 1. With the shortcut the scaled input, nothing packed. Without it two fp32 tensors and a bf16 one (which
    travels uncompressed) in one round follow the rule, the residual carried from step to step under a name until
    the name comes back from Compression.topk or reset_error_feedback() raises the epoch."""
    from ddl.torch import Compression, communicator
    from ddl.torch.compression import reset_error_feedback
    from ddl.torch.tensor_communicate import allreduce_async, allreduce_async_batch
    world = communicator.Communicator.world()
    gs = [np.random.default_rng(7 + i).standard_normal(n).astype(np.float32) for i, n in enumerate((4099, 300))]
    ts, half = [torch.from_numpy(g).cuda() for g in gs], torch.arange(9, device='cuda').bfloat16()
    out = allreduce_async(ts[0], 'sign1/short', world, compression=Compression.onebit, prescale=2.0, postscale=0.125).wait(60)
    assert torch.equal(out, ts[0] * 0.25)

    def step(compression=Compression.onebit):
        hs = allreduce_async_batch(ts + [half], ['sign1/a', 'sign1/b', 'sign1/h'], world, compression=compression)
        got = [h.wait(60) for h in hs]
        assert torch.equal(got[2], half)
        return [g.cpu().numpy().tobytes() for g in got[:2]]

    with config(lib, one_rank_shortcut=0):
        first = [reference([g], [np.zeros(g.size, np.float32)]) for g in gs]
        second = [reference([g], kept)[0].tobytes() for g, (_, kept) in zip(gs, first)]
        first = [out.tobytes() for out, _ in first]
        assert first != second and [step(), step()] == [first, second]
        step(Compression.topk)
        assert [step(), step()] == [first, second]  # back from another family of wire: from zero
        reset_error_feedback()
        assert step() == first


def test_sign_over_multirank_rccl(gpu, monkeypatch):
    monkeypatch.setattr(_mp_gpu_worker, 'worker', _sign_helpers.worker)  # what _run spawns, with 'rccl'
    assert all([n for n, _, _ in results] == ['check_sign_batch'] for results in _run(2, ['check_sign_batch']).values())
