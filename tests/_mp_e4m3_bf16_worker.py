"""Worker of tests/test_e4m3_bf16_multiproc_gpu.py: its checks, added to tests/_mp_gpu_worker.worker's table inside the
child. Every rank runs the CPU model (tests/_e4m3_bf16_helpers.py) for ALL ranks' inputs and compares its bits with
rank 0's. Test infrastructure only."""
import math
import struct

import numpy as np

import _e4m3_bf16_helpers as hb
import _e4m3_helpers as q8
import _mp_gpu_worker
from _bf16_native_helpers import assert_same, same_double
from _mp_e4m3_worker import THIRD
from _mp_stack_worker import _raw
from _mp_sumsq_worker import _same_as_rank0


def _bits(t):
    import torch
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16).reshape(-1)


def check_e4m3_bf16_mixed_batch(ctx):
    """One AVG batch under Compression.fp8_all: bf16 tensors (one cut by 64 KiB sub-plans; factors and the statistic per
    request), an fp32 tensor, and an fp16 tensor, which travels uncompressed."""
    import _avg_helpers as a
    import _helpers as h
    torch, lib, comm, P, r, ora = ctx['torch'], ctx['lib'], ctx['comm'], ctx['P'], ctx['rank'], ctx['oracle']
    from ddl.torch import Compression, cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async_batch
    elems, pre, post = [5, 253, 70_001, 1009], [1.0, THIRD, 0.5, 1.0], [1.0, 1.0, THIRD, 3.0]
    k = len(elems)
    xs = [[hb.rank_input(n, 700 + i, q, specials=i < 2) for i, n in enumerate(elems)] for q in range(P)]
    f32 = [q8.rank_input(4099, 750, q, specials=False) for q in range(P)]
    f16 = [h.random_input(h.DT_HALF, 333, 760 + q) for q in range(P)]
    with h.config(lib, fusion_pipeline_bytes=64 << 10):
        ts = [torch.from_numpy(x.view(np.int16)).cuda().view(torch.bfloat16) for x in xs[r]]
        ts += [torch.from_numpy(f32[r]).cuda(), torch.from_numpy(f16[r]).cuda()]
        hs = allreduce_async_batch(ts, [f'q16mp_{i}' for i in range(k + 2)], comm, op=cb.OP_AVG,
                                   compression=Compression.fp8_all, prescale=pre + [1.0, 1.0], postscale=post + [1.0, 1.0],
                                   sumsq=[True] * k + [False, False])
        got = [hd.wait(timeout=120) for hd in hs]
    cuts = q8.subplan_cuts(elems, 64 << 10)  # the bf16 requests are one plan of their own, in key order
    assert cuts[2] and not cuts[3]
    for i in range(k):
        assert_same(_bits(got[i]), hb.allreduce([xs[q][i] for q in range(P)], q8.OP_AVG, pre[i], post[i]), f'bf16 request {i}')
        assert same_double(hs[i].sumsq, hb.sumsq(_bits(got[i]), cuts[i])), (i, hs[i].sumsq)
    a.assert_same(h.DT_FLOAT, got[k].cpu().numpy(), q8.allreduce(f32, q8.OP_AVG), 'the fp32 tensor of the batch')
    a.assert_same(h.DT_HALF, got[k + 1].cpu().numpy(), a.quotient(h.DT_HALF, ora.fold_ref_order(h.DT_HALF, f16), P),
                  'the fp16 tensor of the batch')
    _same_as_rank0(ctx, _raw([_bits(g) for g in got[:k]]), 'e4m3 bf16 mixed batch')


def check_e4m3_bf16_wrapper(ctx):
    """The data-parallel wrapper on a small bf16 MLP with Compression.fp8_all, fused_mean and track_grad_norm, two steps.
    The ranks' raw gradients are exchanged over the test's gloo group before each step; after it every p.grad is the
    model's bits and grad_norm is sqrt(fsum(the stored bf16 values' sums of squares)) as a double."""
    import _helpers as h
    import _stack_helpers as sh
    torch, lib, comm, P, r, dist = (ctx[k] for k in ('torch', 'lib', 'comm', 'P', 'rank', 'dist'))
    from ddl.torch import Compression
    from ddl.torch.parallelism.data.distributed_optimizer import data_parallelism_distributed_optimizer_wrapper as wrap
    raw = b''
    with h.config(lib, fusion_pipeline_bytes=0):
        model = sh.mlp(torch, 'cuda').to(torch.bfloat16)
        opt = wrap(torch.optim.SGD(model.parameters(), lr=0.1), comm, bucket_bytes=None, compression=Compression.fp8_all,
                   fused_mean=True, track_grad_norm=True)
        params, gen = list(model.parameters()), sh.shard(torch, r)
        for t in range(2):
            opt.zero_grad()
            x, y = (torch.randn(8, d, generator=gen).cuda().to(torch.bfloat16) for d in (16, 4))
            torch.nn.functional.mse_loss(model(x), y).backward()
            want = []
            for p in params:
                g = p.grad.detach().float().cpu().contiguous()  # widened (exact): gloo takes no 16-bit integers
                parts = [torch.empty_like(g) for _ in range(P)]
                dist.all_gather(parts, g)
                want.append(hb.allreduce([(q.numpy().reshape(-1).view(np.uint32) >> 16).astype(np.uint16) for q in parts], q8.OP_AVG))
            opt.step()
            seen = [_bits(p.grad) for p in params]
            assert all(s.tobytes() == w.tobytes() for s, w in zip(seen, want)), f'step {t + 1}'
            norm = math.sqrt(math.fsum(hb.sumsq(w) for w in want))
            assert struct.pack('<d', opt.grad_norm) == struct.pack('<d', norm), (t, opt.grad_norm, norm)
            raw += _raw(seen) + struct.pack('<d', opt.grad_norm)
    _same_as_rank0(ctx, raw, 'e4m3 bf16 wrapper')


def worker(rank, world, port, q, only, transport):
    _mp_gpu_worker.FAULT_CHECKS.update({f.__name__: f for f in (check_e4m3_bf16_mixed_batch, check_e4m3_bf16_wrapper)})
    _mp_gpu_worker.worker(rank, world, port, q, only=only, transport=transport)
