"""DDL_ALLREDUCE_OP_ADASUM through the engine on one GPU: the one-rank world, the refusals, whole-tensor plans."""
import ctypes

import pytest
import torch

from _adasum_helpers import random_inputs, run_thread_adasum
from _helpers import DT_BFLOAT16, DT_DOUBLE, DT_FLOAT, DT_HALF, config

pytestmark = pytest.mark.gpu
VP, SZ, INVALID, ADASUM = ctypes.c_void_p, ctypes.c_size_t, 3, 6
FLAGS = (0x100, 0x200, 0x1100, 0x1000, 0x8200, 0x8000, 0x20000, 0x60000, 0x40000, 0x2000)  # wire bits, SUMSQ


@pytest.mark.parametrize('shortcut', [0, 1])
def test_one_rank_world_is_the_scaled_input(gpu, lib, shortcut):
    """P = 1 under a threshold below one tensor: the input, the factors applied as SUM applies them."""
    from ddl.torch import cpp_backend as cb
    from ddl.torch.communicator import Communicator
    from ddl.torch.tensor_communicate import allreduce_async, allreduce_async_batch
    ts, world = [torch.randn(n, device='cuda') for n in (1, 65, 4099, 70_001)], Communicator.world()
    with config(lib, one_rank_shortcut=shortcut, fusion_threshold_bytes=1024):
        hs = allreduce_async_batch(ts, [f'ada1_{shortcut}_{i}' for i in range(4)], world, op=cb.OP_ADASUM)
        hs.append(allreduce_async(ts[2], f'ada1_{shortcut}', world, op=cb.OP_ADASUM, prescale=2.0, postscale=0.125))
        assert all(torch.equal(h.wait(60), t) for t, h in zip(ts + [ts[2] * 0.25], hs))


def test_refusals(gpu, lib):
    """INVALID_ARGUMENT and a ddl_last_error text, nothing registered; Python: ValueError (here: device tensors)."""
    from ddl.torch import cpp_backend as cb
    from ddl.torch.communicator import Communicator
    from ddl.torch.tensor_communicate import allreduce, allreduce_async
    done, s, world = cb.DONE_FN(lambda status, user: None), torch.cuda.current_stream().cuda_stream, Communicator.world()
    d, h = torch.ones(16, device='cuda'), torch.ones(16)
    n1, keys = (SZ * 1)(16), (ctypes.c_char_p * 1)(b'refused')
    arg = cb.SumsqArg(None, None)  # what the SUMSQ bit makes of `user`
    users = (VP * 1)(ctypes.addressof(arg))
    cases = [(ADASUM, dt, d) for dt in (DT_HALF, DT_BFLOAT16, DT_DOUBLE)] + [(ADASUM, DT_FLOAT, h)]
    for op, dt, t in cases + [(ADASUM | f, DT_FLOAT, d) for f in FLAGS]:
        p, arr, mem = t.data_ptr(), (VP * 1)(t.data_ptr()), cb.MEMORY_DEVICE if t.is_cuda else cb.MEMORY_HOST
        assert lib.ddl_allreduce_submit_mem(world.id, keys[0], p, p, 16, dt, op, mem, s, done, users[0]) == INVALID, (op, dt)
        assert lib.ddl_allreduce_submit_batch_mem(world.id, 1, keys, arr, arr, n1, (ctypes.c_int * 1)(dt), op, mem, s, done,
                                                  users) == INVALID and lib.ddl_last_error(), (op, dt)
    p, one, many = d.data_ptr(), (VP * 1)(d.data_ptr()), (VP * 17)(*([d.data_ptr()] * 17))
    assert [lib.ddl_allreduce(world.id, p, p, 16, DT_FLOAT, ADASUM, s),
            lib.ddl_allreduce_batch(world.id, 1, one, one, n1, DT_FLOAT, ADASUM, s),
            lib.ddl_allreduce_host(world.id, h.data_ptr(), h.data_ptr(), 16, DT_FLOAT, ADASUM),
            lib.ddl_allreduce_variant(world.id, p, p, 16, DT_FLOAT, ADASUM, s, 0),
            lib.ddl_local_ring_allreduce(1, one, one, 16, DT_FLOAT, ADASUM, s),
            lib.ddl_testing_thread_adasum(17, 1, many, many, n1, None, None, s)] == [INVALID] * 6  # the last: 17 ranks
    for t in (d.bfloat16(), torch.ones(4, 4, device='cuda').t()):
        with pytest.raises(ValueError):
            allreduce_async(t, 'refused', world, op=cb.OP_ADASUM)
    assert lib.ddl_wait_all(world.id) == 0  # nothing was registered
    assert torch.equal(allreduce(d, world), d)  # a SUM still works


def test_a_small_fusion_threshold_cuts_no_tensor(lib, gpu):
    """P = 2, every request a plan of its own (64 bytes) or the group split (1200): bit for bit the uncut result."""
    xs = random_inputs(2)
    whole = run_thread_adasum(lib, xs)
    for threshold in (64, 1200):
        with config(lib, fusion_threshold_bytes=threshold):
            cut = run_thread_adasum(lib, xs)
        assert all(a.tobytes() == b.tobytes() for r in range(2) for a, b in zip(cut[r], whole[r])), threshold
