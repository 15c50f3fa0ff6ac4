"""DDL_ALLREDUCE_WIRE_LOWRANK on the GPU. The kernels (csrc/lowrank.hip) through ddl_testing_thread_lowrank against the
NumPy rule of _lowrank_helpers in fp64, within 4 times what fp32 costs that same restatement on the same inputs (the
floor; DESIGN 5.16 records the largest); the engine: the refusals, the config key, a mixed round on the keyed path, the
restarts of e and Q, the one-rank shortcut, and P = 2 processes over RCCL (_lowrank_helpers.check_lowrank_batch)."""
import ctypes

import numpy as np
import pytest
import torch

import _lowrank_helpers
import _mp_gpu_worker
from _helpers import DT_BFLOAT16, DT_DOUBLE, DT_FLOAT, DT_HALF, config
from _lowrank_helpers import AVG, LENGTHS, NAN, SUM, State, close, device_state, rel, run_thread_lowrank, signal, step
from test_multiproc_rccl_gpu import _run

pytestmark = pytest.mark.gpu
VP, SZ, INVALID, UNSUPPORTED_DTYPE, LOWRANK = ctypes.c_void_p, ctypes.c_size_t, 3, 4, 0x200000
# every other wire, feedback and stochastic bit, SUMSQ, and the ops MIN, MAX, ADASUM
FLAGS = (0x100, 0x200, 0x1000, 0x1100, 0x8000, 0x8200, 0x20000, 0x40000, 0x60000, 0x80000, 0x100000, 0x2000, 3, 4, 6)
CASES = [(P, op, r, 'normal') for P in (1, 2, 3, 8) for op in (SUM, AVG) for r in (1, 3, 4, 16)]
CASES += [(3, op, r, family) for family in ('offset', 'scaled') for op in (SUM, AVG) for r in (1, 3, 4, 16)]


def fresh(lib, lengths, P, off=0):  # res[q][i], qs[q][i]: zeroed residuals and Q states between guards
    dev = [device_state(lib, n, P, off) for n in lengths]
    return [[[d[k][q] for d in dev] for q in range(P)] for k in range(2)]


def by_rank(xs):
    return [list(row) for row in zip(*xs)]  # xs[i][q] -> [q][i]


@pytest.mark.parametrize('P,op,r,family', CASES)
def test_two_steps_of_one_plan_against_the_rule(lib, gpu, P, op, r, family):
    """offset: everything 4 bytes off a 16-byte boundary. scaled: prescale 0.3, postscale 1.7. The first AVG step
    also shows the compensation: |sum e' + P out - sum a| <= 2^-24 sum |e'|, one rounding per rank's subtraction."""
    (pre, post), off = (0.3, 1.7) if family == 'scaled' else (None, None), int(family == 'offset')
    with config(lib, wire_lowrank_rank=r):
        (res, qs), st64, st32 = fresh(lib, LENGTHS, P, off), *[[State(n, r, P) for n in LENGTHS] for _ in range(2)]
        for it in range(2):
            xs = [signal(n, r, P, 1000 * it + 10 * P + i) for i, n in enumerate(LENGTHS)]
            outs = run_thread_lowrank(lib, by_rank(xs), res, qs, op, pre, post, off)
            for i, n in enumerate(LENGTHS):
                want, a = step(xs[i], st64[i], r, op, pre or 1.0, post or 1.0)
                floor = rel(step(xs[i], st32[i], r, op, pre or 1.0, post or 1.0, dt=np.float32)[0], want)
                small = st64[i].small
                assert all(outs[q][i].tobytes() == outs[0][i].tobytes() for q in range(P)), (it, n, 'ranks differ')
                assert close(outs[0][i], want, floor, a if small else None, post or 1.0), (it, n, 'out')
                if small:
                    continue
                kept = [res[q][i].cpu().numpy() for q in range(P)]
                floor = max(rel(st32[i].e[q], st64[i].e[q].astype(np.float64)) for q in range(P))
                assert all(close(kept[q], st64[i].e[q].astype(np.float64), floor) for q in range(P)), (it, n, 'residual')
                assert all(qs[q][i].cpu().numpy().tobytes() == qs[0][i].cpu().numpy().tobytes() for q in range(P))
                if op == AVG and pre is None and it == 0:  # (a = g exactly)
                    gap = np.sum(kept, axis=0, dtype=np.float64) + P * outs[0][i].astype(np.float64) - np.sum(a, axis=0, dtype=np.float64)
                    assert (np.abs(gap) <= 2.0 ** -24 * np.sum(np.abs(kept), axis=0, dtype=np.float64)).all(), (n, 'compensation')


@pytest.mark.parametrize('n', [4096, 1 << 20])
def test_a_sum_of_rank_r_comes_back_after_one_step(lib, gpu, n):
    """P = 3, r = 4, n = R C, small-integer factors: the ranks' a and their sum are exact in fp32, of rank 4 exactly.
    SUM's out is that sum, and the ranks' e' sum to zero, to the bound of the test above."""
    R, C, _ = _lowrank_helpers.shape(n, 4)
    v = np.random.default_rng(n).integers(-3, 4, (C, 4))
    gs = [(np.random.default_rng(n + q).integers(-3, 4, (R, 4)) @ v.T).reshape(-1).astype(np.float32) for q in range(3)]
    total = np.sum(gs, axis=0, dtype=np.float64)
    res, qs = fresh(lib, [n], 3)
    out = run_thread_lowrank(lib, [[g] for g in gs], res, qs)[0][0]
    floor = rel(step(gs, State(n, 4, 3), 4, dt=np.float32)[0], step(gs, State(n, 4, 3), 4)[0])
    assert rel(out, total) <= 4 * floor
    assert np.abs(np.sum([r[0].cpu().numpy() for r in res], axis=0, dtype=np.float64)).max() <= 4 * floor * np.abs(total).max()


def test_runs_repeat_zero_steps_reseed_and_a_nan_poisons(lib, gpu):
    """P = 2, r = 4. An all-zero step leaves the whole state zero and the next step equals a first step, bit for bit.
    A NaN on rank 0 at the second step: NaN in all of out on every rank; e, Q and the flags as before the step."""
    lengths = (4099, 70001)
    xs = by_rank([signal(n, 4, 2, 7 + i) for i, n in enumerate(lengths)])
    res, qs = fresh(lib, lengths, 2)
    first = [o.tobytes() for row in run_thread_lowrank(lib, xs, res, qs) for o in row]
    res2, qs2 = fresh(lib, lengths, 2)
    zeros = run_thread_lowrank(lib, [[np.zeros_like(x) for x in row] for row in xs], res2, qs2)
    assert all(not o.any() for row in zeros for o in row) and all(not t.any() for ts in (res2, qs2) for row in ts for t in row)
    assert [o.tobytes() for row in run_thread_lowrank(lib, xs, res2, qs2) for o in row] == first
    before = [t.cpu().numpy().tobytes() for ts in (res, qs) for row in ts for t in row]
    assert any(t.any() for row in qs for t in row)
    bad = [[x.copy() for x in row] for row in xs]
    for x in bad[0]:
        x[5] = np.nan
    outs = run_thread_lowrank(lib, bad, res, qs)
    assert all((o.view(np.uint32) == NAN).all() for row in outs for o in row)
    assert [t.cpu().numpy().tobytes() for ts in (res, qs) for row in ts for t in row] == before


def test_refusals_and_the_config_key(gpu, lib):
    """Before anything is registered; the communicator works afterwards."""
    from ddl.torch import cpp_backend as cb
    from ddl.torch.communicator import Communicator
    from ddl.torch.tensor_communicate import allreduce
    done, s, world = cb.DONE_FN(lambda status, user: None), torch.cuda.current_stream().cuda_stream, Communicator.world()
    d, h = torch.ones(16, device='cuda'), torch.ones(16)
    n1, keys = (SZ * 1)(16), (ctypes.c_char_p * 1)(b'refused')
    arg = cb.SumsqArg(None, None)  # what the SUMSQ bit makes of `user`
    users = (VP * 1)(ctypes.addressof(arg))
    cases = [(LOWRANK, dt, d, UNSUPPORTED_DTYPE) for dt in (DT_HALF, DT_BFLOAT16, DT_DOUBLE)] + [(LOWRANK, DT_FLOAT, h, INVALID)]
    for op, dt, t, status in cases + [(LOWRANK | f, DT_FLOAT, d, INVALID) for f in FLAGS]:
        p, arr, mem = t.data_ptr(), (VP * 1)(t.data_ptr()), cb.MEMORY_DEVICE if t.is_cuda else cb.MEMORY_HOST
        assert lib.ddl_allreduce_submit_mem(world.id, keys[0], p, p, 16, dt, op, mem, s, done, users[0]) == status, (op, dt)
        assert lib.ddl_allreduce_submit_batch_mem(world.id, 1, keys, arr, arr, n1, (ctypes.c_int * 1)(dt), op, mem,
                                                  s, done, users) == status and lib.ddl_last_error(), (op, dt)
    p, one = d.data_ptr(), (VP * 1)(d.data_ptr())
    assert [lib.ddl_allreduce_submit_mem(world.id, keys[0], p, p, 1 << 31, DT_FLOAT, LOWRANK, cb.MEMORY_DEVICE, s, done, None),
            lib.ddl_allreduce(world.id, p, p, 16, DT_FLOAT, LOWRANK, s),
            lib.ddl_allreduce_batch(world.id, 1, one, one, n1, DT_FLOAT, LOWRANK, s),
            lib.ddl_allreduce_host(world.id, h.data_ptr(), h.data_ptr(), 16, DT_FLOAT, LOWRANK)] == [INVALID] * 4
    assert lib.ddl_wait_all(world.id) == 0  # nothing was registered
    assert torch.equal(allreduce(d, world), d)  # a SUM still works
    assert [lib.ddl_set_config(b'wire_lowrank_rank', v) for v in (0, -1, 17)] == [INVALID] * 3
    assert lib.ddl_get_config(b'wire_lowrank_rank') == 4


def test_a_mixed_round_and_the_restarts(gpu, lib):
    """P = 1. With the shortcut the scaled input. Without it two fp32 tensors and a bf16 one (uncompressed) in one round
    follow the rule; reset_error_feedback() restarts e and NOT Q; names coming back with other sizes restart both."""
    from ddl.torch import Compression, communicator
    from ddl.torch.compression import reset_error_feedback
    from ddl.torch.tensor_communicate import allreduce_async, allreduce_async_batch
    world, half = communicator.Communicator.world(), torch.arange(9, device='cuda').bfloat16()
    t = torch.randn(4099, device='cuda')
    out = allreduce_async(t, 'lr1/short', world, compression=Compression.powersgd, prescale=2.0, postscale=0.125).wait(60)
    assert torch.equal(out, t * 0.25)

    def steps(lengths, count, st=None, reset=False):
        # plain normal gradients: no low rank to find, so a wrong e or Q shows in full
        gs = [np.random.default_rng(7 + i).standard_normal(n).astype(np.float32) for i, n in enumerate(lengths)]
        st = st or [[State(n, 4, 1) for n in lengths] for _ in range(2)]
        for pair in st if reset else []:
            for one in pair:
                one.e = [np.zeros_like(one.e[0])]
        for _ in range(count):
            hs = allreduce_async_batch([torch.from_numpy(g).cuda() for g in gs] + [half], ['lr1/a', 'lr1/b', 'lr1/h'], world,
                                       compression=Compression.powersgd)
            got = [h.wait(60) for h in hs]
            assert torch.equal(got[2], half)
            for i, g in enumerate(gs):
                want = step([g], st[0][i], 4)[0]
                assert close(got[i].cpu().numpy(), want, rel(step([g], st[1][i], 4, dt=np.float32)[0], want)), (lengths, i)
        return st

    with config(lib, one_rank_shortcut=0):
        st = steps((4099, 70001), 2)
        reset_error_feedback()
        steps((4099, 70001), 1, st, reset=True)
        steps((4100, 70002), 2)


def test_lowrank_over_multirank_rccl(gpu, monkeypatch):
    monkeypatch.setattr(_mp_gpu_worker, 'worker', _lowrank_helpers.worker)  # what _run spawns, with 'rccl'
    assert all([n for n, _, _ in results] == ['check_lowrank_batch'] for results in _run(2, ['check_lowrank_batch']).values())
