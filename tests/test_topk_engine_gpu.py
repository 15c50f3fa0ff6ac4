"""DDL_ALLREDUCE_WIRE_TOPK through the engine on one GPU: the refusals, the density's range, whole-tensor plans,
the residual's restart and the one-rank world."""
import ctypes

import numpy as np
import pytest
import torch

from _helpers import DT_BFLOAT16, DT_DOUBLE, DT_FLOAT, DT_HALF, config
from _topk_helpers import LENGTHS, reference, run_thread_topk

pytestmark = pytest.mark.gpu
VP, SZ, INVALID, UNSUPPORTED_DTYPE, TOPK = ctypes.c_void_p, ctypes.c_size_t, 3, 4, 0x80000
# every other wire, feedback and stochastic bit, SUMSQ, and the ops MIN, MAX, ADASUM
FLAGS = (0x100, 0x200, 0x1000, 0x1100, 0x8000, 0x8200, 0x20000, 0x40000, 0x60000, 0x2000, 3, 4, 6)


def test_refusals(gpu, lib):
    """Before anything is registered; the Python ValueErrors; the density's range."""
    from ddl.torch import Compression, cpp_backend as cb
    from ddl.torch.communicator import Communicator
    from ddl.torch.tensor_communicate import allreduce, allreduce_async, allreduce_gradient
    done, s, world = cb.DONE_FN(lambda status, user: None), torch.cuda.current_stream().cuda_stream, Communicator.world()
    d, h = torch.ones(16, device='cuda'), torch.ones(16)
    n1, keys = (SZ * 1)(16), (ctypes.c_char_p * 1)(b'refused')
    arg = cb.SumsqArg(None, None)  # what the SUMSQ bit makes of `user`
    users = (VP * 1)(ctypes.addressof(arg))
    cases = [(TOPK, dt, d, 16, UNSUPPORTED_DTYPE) for dt in (DT_HALF, DT_BFLOAT16, DT_DOUBLE)]
    cases += [(TOPK, DT_FLOAT, h, 16, INVALID), (TOPK, DT_FLOAT, d, 1 << 31, INVALID)]
    for op, dt, t, n, status in cases + [(TOPK | f, DT_FLOAT, d, 16, INVALID) for f in FLAGS]:
        p, arr, mem = t.data_ptr(), (VP * 1)(t.data_ptr()), cb.MEMORY_DEVICE if t.is_cuda else cb.MEMORY_HOST
        assert lib.ddl_allreduce_submit_mem(world.id, keys[0], p, p, n, dt, op, mem, s, done, users[0]) == status, (op, dt)
        assert lib.ddl_allreduce_submit_batch_mem(world.id, 1, keys, arr, arr, (SZ * 1)(n), (ctypes.c_int * 1)(dt), op, mem,
                                                  s, done, users) == status and lib.ddl_last_error(), (op, dt)
    p, one = d.data_ptr(), (VP * 1)(d.data_ptr())
    assert [lib.ddl_allreduce(world.id, p, p, 16, DT_FLOAT, TOPK, s),
            lib.ddl_allreduce_batch(world.id, 1, one, one, n1, DT_FLOAT, TOPK, s),
            lib.ddl_allreduce_host(world.id, h.data_ptr(), h.data_ptr(), 16, DT_FLOAT, TOPK)] == [INVALID] * 3
    with pytest.raises(ValueError):
        allreduce_async(d, 'refused', world, compression=Compression.topk, sumsq=True)
    with pytest.raises(ValueError):
        allreduce_gradient(d, world, compression=Compression.topk)
    assert [lib.ddl_set_config(b'wire_topk_ppm', v) for v in (0, -1, 1_000_001)] == [INVALID] * 3
    assert lib.ddl_get_config(b'wire_topk_ppm') == 10_000
    assert lib.ddl_wait_all(world.id) == 0  # nothing was registered
    assert torch.equal(allreduce(d, world), d)  # a SUM still works


def test_a_small_fusion_threshold_cuts_no_tensor(lib, gpu):
    """P = 2, every request a plan of its own (64 bytes) or the group split (1200): the bits of the uncut run."""
    xs = [[np.random.default_rng(50 * r + i).standard_normal(n).astype(np.float32) for i, n in enumerate(LENGTHS)]
          for r in range(2)]
    runs = []
    for threshold in (None, 64, 1200):
        res = [[torch.zeros(n, device='cuda') for n in LENGTHS] for _ in range(2)]
        with config(lib, **({} if threshold is None else {'fusion_threshold_bytes': threshold})):
            outs = run_thread_topk(lib, xs, res)
        runs.append([o.tobytes() for row in outs for o in row] + [t.cpu().numpy().tobytes() for row in res for t in row])
    assert runs[1] == runs[0] and runs[2] == runs[0]


def test_one_rank_world_and_the_residuals_restart(gpu, lib):
    """P = 1: with the shortcut the scaled input, nothing selected; without it the rule, the residual carried from
    step to step under a name until reset_error_feedback() restarts it."""
    from ddl.torch import Compression
    from ddl.torch.communicator import Communicator
    from ddl.torch.compression import reset_error_feedback
    from ddl.torch.tensor_communicate import allreduce_async
    world, g = Communicator.world(), np.random.default_rng(7).standard_normal(4099).astype(np.float32)
    t, zero = torch.from_numpy(g).cuda(), np.zeros(4099, np.float32)
    out = allreduce_async(t, 'topk1/short', world, compression=Compression.topk, prescale=2.0, postscale=0.125).wait(60)
    assert torch.equal(out, t * 0.25)
    with config(lib, one_rank_shortcut=0):
        first, kept = reference([g], [zero], 10_000)
        second, _ = reference([g], kept, 10_000)
        got = [allreduce_async(t, 'topk1/kept', world, compression=Compression.topk).wait(60).cpu().numpy() for _ in range(2)]
        assert [x.tobytes() for x in got] == [first.tobytes(), second.tobytes()] and first.tobytes() != second.tobytes()
        reset_error_feedback()
        again = allreduce_async(t, 'topk1/kept', world, compression=Compression.topk).wait(60).cpu().numpy()
        assert again.tobytes() == first.tobytes()
