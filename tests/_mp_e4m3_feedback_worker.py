"""Worker of tests/test_e4m3_feedback_multiproc_gpu.py: error feedback of the e4m3 wire
(DDL_ALLREDUCE_WIRE_E4M3_FEEDBACK) on the whole engine in several processes on one GPU. The process setup is
tests/_mp_gpu_worker.worker, unchanged; this module only adds its checks to that worker's table inside the child.
Every rank runs the CPU model (tests/_e4m3_feedback_helpers.py) for ALL ranks' inputs and also compares its bits with
rank 0's. Test infrastructure only."""
import math
import struct

import numpy as np

import _e4m3_feedback_helpers as fb
import _e4m3_helpers as q8
import _mp_gpu_worker
from _mp_stack_worker import _raw
from _mp_sumsq_worker import _same_as_rank0

THIRD = float(np.float32(1) / np.float32(3))
ELEMS = [5, 253, 70_001, 1009]
PRE, POST = [1.0, THIRD, 0.5, 1.0], [1.0, 1.0, THIRD, 3.0]


def _steps(ctx, tag, seed, mine, feedback):
    """Two steps of one batch under stable names (64 KiB sub-plans cut the 70_001-element request); this rank sends
    with compression `mine`, the model has rank q carry the bit where feedback[q]."""
    import _avg_helpers as a
    import _helpers as h
    torch, lib, comm, P, r = ctx['torch'], ctx['lib'], ctx['comm'], ctx['P'], ctx['rank']
    from ddl.torch import cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async_batch
    xs = [[[q8.rank_input(n, seed + 50 * t + i, q, specials=t == 0 and i < 2) for i, n in enumerate(ELEMS)]
           for q in range(P)] for t in range(2)]
    want = [fb.allreduce_steps([[xs[t][q][i] for q in range(P)] for t in range(2)], q8.OP_AVG, PRE[i], POST[i],
                               feedback=feedback)[0] for i in range(len(ELEMS))]
    raw = b''
    with h.config(lib, fusion_pipeline_bytes=64 << 10):
        for t in range(2):
            ts = [torch.from_numpy(x).cuda() for x in xs[t][r]]
            hs = allreduce_async_batch(ts, [f'{tag}_{i}' for i in range(len(ELEMS))], comm, op=cb.OP_AVG,
                                       compression=mine, prescale=PRE, postscale=POST)
            for i, hd in enumerate(hs):
                out = hd.wait(timeout=120).cpu().numpy()
                a.assert_same(h.DT_FLOAT, out, want[i][t], f'{tag} step {t} request {i} ({ELEMS[i]} elements)')
                raw += _raw([out])
    return raw, want


def check_e4m3_fb_steps(ctx):
    """Two steps under stable names: the model's bits on every rank, and the same bytes as rank 0."""
    from ddl.torch import Compression
    raw, _ = _steps(ctx, 'q8fbmp', 700, Compression.fp8_feedback, None)
    _same_as_rank0(ctx, raw, 'e4m3 feedback steps')


def check_e4m3_fb_disagree(ctx):
    """The last rank sends without the bit: the bit is rank-local, so nothing hangs and every rank gets the numbers
    of the model in which that rank keeps no residual — other numbers than with the bit on every rank."""
    from ddl.torch import Compression
    P, r = ctx['P'], ctx['rank']
    mask = [q != P - 1 for q in range(P)]
    raw, want = _steps(ctx, 'q8fbmp_dis', 800, Compression.fp8_feedback if mask[r] else Compression.fp8, mask)
    xs = [[q8.rank_input(ELEMS[2], 800 + 50 * t + 2, q, specials=False) for q in range(P)] for t in range(2)]
    agreed = fb.allreduce_steps(xs, q8.OP_AVG, PRE[2], POST[2])[0]
    assert agreed[0].tobytes() == want[2][0].tobytes() and agreed[1].tobytes() != want[2][1].tobytes()
    _same_as_rank0(ctx, raw, 'e4m3 feedback, one rank without the bit')


def check_e4m3_fb_wrapper(ctx):
    """The data-parallel wrapper on a three-parameter fp32 model with Compression.fp8_feedback, fused_mean,
    gradient_predivide_factor 2 and track_grad_norm over two steps, on the step() path and (behind
    reset_error_feedback(): the names are the same) on the overlap_backward hooks. The ranks' raw gradients are
    exchanged over the test's gloo group before each step; after it every p.grad is the model's value bit for bit
    — the second step on the residuals of the first, in prescaled units — and grad_norm is
    sqrt(fsum(uncompressed sums of squares))."""
    import _helpers as h
    from _sumsq_helpers import mirror
    torch, lib, comm, P, r, dist = (ctx[k] for k in ('torch', 'lib', 'comm', 'P', 'rank', 'dist'))
    from ddl.torch import Compression
    from ddl.torch.compression import reset_error_feedback
    from ddl.torch.parallelism.data.distributed_optimizer import data_parallelism_distributed_optimizer_wrapper as wrap
    raw, PF = b'', 2.0
    pre, post = float(np.float32(1.0 / PF)), float(np.float32(PF))
    with h.config(lib, fusion_pipeline_bytes=0):
        for overlap in (False, True):
            reset_error_feedback()
            torch.manual_seed(4321)  # the same weights on every rank
            model = torch.nn.Sequential(torch.nn.Linear(40, 30), torch.nn.Tanh(), torch.nn.Linear(30, 9, bias=False)).cuda()
            opt = wrap(torch.optim.SGD(model.parameters(), lr=0.1), comm, overlap_backward=overlap, bucket_bytes=None,
                       compression=Compression.fp8_feedback, fused_mean=True, gradient_predivide_factor=PF,
                       track_grad_norm=True)
            params = list(model.parameters())
            assert len(params) == 3
            gen = torch.Generator().manual_seed(77 + r)  # its own shard of the batches
            resid = [[np.zeros(p.numel(), np.float32) for p in params] for _ in range(P)]
            for t in range(2):
                what = f'overlap {overlap} step {t + 1}'
                opt.zero_grad()
                x, y = torch.randn(8, 40, generator=gen).cuda(), torch.randn(8, 9, generator=gen).cuda()
                loss = torch.nn.functional.mse_loss(model(x), y)
                if overlap:  # the hooks reduce p.grad in place during backward(): the raw gradients first
                    mine = [g.detach().cpu().contiguous() for g in torch.autograd.grad(loss, params, retain_graph=True)]
                else:
                    loss.backward()
                    mine = [p.grad.detach().cpu().contiguous() for p in params]
                theirs = []  # theirs[i][q]: rank q's gradient of parameter i
                for g in mine:
                    parts = [torch.empty_like(g) for _ in range(P)]
                    dist.all_gather(parts, g)
                    theirs.append([part.numpy().reshape(-1) for part in parts])
                if overlap:
                    loss.backward()
                opt.step()
                seen = [p.grad.detach().cpu().numpy().reshape(-1).copy() for p in params]
                sqs = []
                for i in range(len(params)):
                    outs, res = fb.allreduce_steps([theirs[i]], q8.OP_AVG, pre, post, residuals=[resid[q][i] for q in range(P)])
                    for q in range(P):
                        resid[q][i] = res[q]
                    assert seen[i].tobytes() == outs[0].tobytes(), f'{what}: parameter {i}'
                    sqs.append(mirror(outs[0], False))
                norm = math.sqrt(math.fsum(sqs))
                assert struct.pack('<d', opt.grad_norm) == struct.pack('<d', norm), (what, opt.grad_norm, norm)
                raw += _raw(seen) + struct.pack('<d', opt.grad_norm)
            assert any(x.any() for x in resid[r])  # the second step did run on something
            for hook in getattr(opt, '_hooks', []):
                hook.remove()
    _same_as_rank0(ctx, raw, 'e4m3 feedback wrapper')


E4M3_FB_CHECKS = {f.__name__: f for f in (check_e4m3_fb_steps, check_e4m3_fb_disagree, check_e4m3_fb_wrapper)}


def worker(rank, world, port, q, only, transport):
    _mp_gpu_worker.FAULT_CHECKS.update(E4M3_FB_CHECKS)
    _mp_gpu_worker.worker(rank, world, port, q, only=only, transport=transport)
