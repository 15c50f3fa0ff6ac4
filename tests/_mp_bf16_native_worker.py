"""Worker of tests/test_bf16_native_multiproc_gpu.py: the sum of squares and the scale factors of NATIVE
bfloat16 keyed allreduces on the whole engine in several processes on one GPU. The process setup is
tests/_mp_gpu_worker.worker, unchanged; this module only adds its checks to that worker's table inside the
child. Expected values: the model of _bf16_native_helpers.py over the oracle's sum of every rank's (seeded,
so locally known) contribution in MPICH's order for the dtype group's plan; every rank also compares its
bits with rank 0's. Test infrastructure only."""
import math
import struct

import numpy as np

import _mp_gpu_worker
from _mp_sumsq_worker import _same_as_rank0

SIZES = [1000, 300_000, 5, 70_001, 513, 0, 4099]


def _dev(torch, bits_):
    return torch.from_numpy(np.ascontiguousarray(bits_).view(np.int16)).cuda().view(torch.bfloat16)


def _host(t):
    import torch
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def check_bf16_native_keyed_mix(ctx):
    """One keyed batch that mixes bf16 and fp32 requests with and without factors and the statistic, every rank
    submitting in its own order: SUM and AVG batches; one plan per dtype group (its bytes are the oracle's
    message). Then ranks that pass DIFFERENT postscales: everybody finishes, each with its own factor."""
    import _bf16_native_helpers as bh
    import _helpers as h
    from _scale_helpers import mul, result, same_bits, scale_input
    from _sumsq_helpers import mirror
    torch, lib, comm, P, r, ora = ctx['torch'], ctx['lib'], ctx['comm'], ctx['P'], ctx['rank'], ctx['oracle']
    from ddl.torch import cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async_batch
    k = len(SIZES)
    raw = b''
    with h.config(lib, fusion_pipeline_bytes=0, reference_order=1):
        for name, op, shift in (('avg', cb.OP_AVG, 0), ('sum', cb.OP_SUM, 2)):
            # requests 0 .. k-1 bf16, k .. 2k-1 fp32; request j without any option where j % 4 == 3
            pre, post = bh.mixed_factors(2 * k, shift), bh.mixed_factors(2 * k, shift + 1)
            wish = [j % 3 != 2 for j in range(2 * k)]
            for j in range(3, 2 * k, 4):
                pre[j] = post[j] = np.float32(1)
                wish[j] = False
            sizes = SIZES + SIZES
            xb = [[bh.native_input(n, 31 * i + 7 * q + shift, specials=(i % 2 == 0)) for q in range(P)]
                  for i, n in enumerate(SIZES)]
            xf = [[scale_input(n, 900 + 31 * i + 7 * q + shift, pre[k + i]) for q in range(P)] for i, n in enumerate(SIZES)]
            ts = [_dev(torch, x[r]) for x in xb] + [torch.from_numpy(x[r]).cuda() for x in xf]
            order = [int(i) for i in np.random.default_rng(5 + r).permutation(2 * k)]
            got = allreduce_async_batch([ts[j] for j in order], [f'bnm_{name}_{j:03d}' for j in order], comm,
                                        outputs=[ts[j] for j in order], op=op,
                                        prescale=[float(pre[j]) for j in order], postscale=[float(post[j]) for j in order],
                                        sumsq=[wish[j] for j in order])
            handles = dict(zip(order, got))
            for hh in got:
                hh.wait(timeout=120)
            gb16, gb32 = sum(2 * n for n in SIZES), sum(4 * n for n in SIZES)
            for i in range(k):  # bf16
                out = _host(ts[i])
                model = bh.expected(ora, xb[i], gb16, op, pre[i], post[i])
                bh.assert_same(out, model, f'{name} bf16 request {i} ({SIZES[i]}, pre {pre[i]}, post {post[i]})')
                hh = handles[i]
                assert (hh.sumsq is not None) == wish[i]
                if wish[i]:
                    assert bh.same_double(hh.sumsq, bh.sumsq(out)), (name, i, hh.sumsq, bh.sumsq(out))
                    raw += struct.pack('<d', 0.0 if math.isnan(hh.sumsq) else hh.sumsq)
                nan = (out & 0x7fff) > 0x7f80
                raw += np.where(nan, np.uint16(0), out).tobytes() + nan.tobytes()
            for i in range(k):  # fp32, in the same batch
                j = k + i
                out = ts[j].cpu().numpy()
                total = ora.fold_ref_order(h.DT_FLOAT, [mul(x, pre[j]) for x in xf[i]], gb32)
                assert same_bits(out, result(total, op, P, post[j])), (name, 'fp32', i)
                if wish[j]:
                    m = mirror(out, False)
                    assert bh.same_double(handles[j].sumsq, m), (name, 'fp32', i)
        # rank-local factors: every rank its own postscale on the same sums
        mine = bh.FACTORS[(r + 1) % len(bh.FACTORS)]
        sizes = [70_001, 5, 300]
        xs = [[bh.native_input(n, 17 * i + q, specials=False) for q in range(P)] for i, n in enumerate(sizes)]
        ts = [_dev(torch, x[r]) for x in xs]
        hs = allreduce_async_batch(ts, [f'bnm_dis_{i}' for i in range(3)], comm, outputs=ts, op=cb.OP_AVG,
                                   postscale=float(mine), sumsq=[True, r == 0, False])
        for i, hh in enumerate(hs):
            hh.wait(timeout=120)
            model = bh.expected(ora, xs[i], sum(2 * n for n in sizes), cb.OP_AVG, 1.0, mine)
            assert _host(ts[i]).tobytes() == model.tobytes(), (i, float(mine))
            if hh.sumsq is not None:
                assert bh.same_double(hh.sumsq, bh.sumsq(model))
    _same_as_rank0(ctx, raw, 'bf16 native keyed mix')


def _model(torch):
    torch.manual_seed(1234)  # the same parameters on every rank
    net = torch.nn.Sequential(torch.nn.Linear(257, 300), torch.nn.Tanh(), torch.nn.Linear(300, 10))
    return net.cuda().to(torch.bfloat16)


def _backward(torch, model, r, scale=1.0, inject=None):
    g = torch.Generator().manual_seed(77 + r)  # every rank its own shard
    x = torch.randn(64, 257, generator=g).cuda().to(torch.bfloat16)
    model.zero_grad()
    loss = model(x).float().pow(2).mean()
    if inject is not None:
        loss = loss * inject
    (loss * scale if not callable(scale) else scale(loss)).backward()


def _gather_grads(torch, dist, model, P):
    """Every rank's local gradients as bf16 bits, through torch.distributed on the host (not the engine)."""
    out = []
    for p in model.parameters():
        mine = p.grad.detach().contiguous().view(torch.int16).cpu().to(torch.int32)  # (gloo has no 16-bit integers)
        all_ = [torch.empty_like(mine) for _ in range(P)]
        dist.all_gather(all_, mine)
        out.append([t.to(torch.int16).numpy().view(np.uint16).ravel() for t in all_])
    return out


def check_bf16_native_wrapper(ctx):
    """The data-parallel wrapper on a bf16 MLP with fused_mean, gradient_predivide_factor = 2, loss_scale = 1024,
    track_grad_norm / max_grad_norm, on the step() path and the overlap_backward hooks, with the torch fall-back
    of the statistic patched to raise: the gradients and grad_norm are the model's over every rank's local
    gradients, grad_norm the same double on every rank; a step with an injected inf is skipped and
    DynamicLossScaler halves its scale."""
    import _bf16_native_helpers as bh
    import _helpers as h
    torch, lib, comm, P, r, ora, dist = (ctx['torch'], ctx['lib'], ctx['comm'], ctx['P'], ctx['rank'], ctx['oracle'],
                                         ctx['dist'])
    from ddl.torch.parallelism.data import DynamicLossScaler
    from ddl.torch.parallelism.data import distributed_optimizer as do
    wrap = do.data_parallelism_distributed_optimizer_wrapper
    assert P == 2  # (the sum of two values has one order: the hooks' plans need no message size)

    def boom(g):
        raise AssertionError(f'the torch fall-back of the statistic ran for a {g.dtype} gradient')
    old = do.DataParallelismDistributedOptimizer._torch_sumsq
    do.DataParallelismDistributedOptimizer._torch_sumsq = staticmethod(boom)
    S, f = 1024.0, 2.0
    raw = b''
    try:
        with h.config(lib, fusion_pipeline_bytes=0):
            for overlap in (False, True):
                def make(**kw):
                    model = _model(torch)
                    opt = wrap(torch.optim.SGD(model.parameters(), lr=0.05), comm, overlap_backward=overlap,
                               bucket_bytes=None, fused_mean=True, gradient_predivide_factor=f, **kw)
                    return model, opt

                def drop(opt):
                    for hook in getattr(opt, '_hooks', []):
                        hook.remove()
                # the local gradients of every rank, from a model without a wrapper
                model = _model(torch)
                _backward(torch, model, r, scale=S)
                local = _gather_grads(torch, dist, model, P)
                gb = sum(2 * g[0].size for g in local)
                want = [bh.expected(ora, g, gb, bh.OP_AVG, np.float32(1.0 / f), np.float32(f * (1.0 / S))) for g in local]
                norm = math.sqrt(math.fsum(bh.sumsq(g) for g in want))
                assert math.isfinite(norm) and norm > 0.0

                model, opt = make(track_grad_norm=True, max_grad_norm=1e30)
                opt.loss_scale = S
                _backward(torch, model, r, scale=S)
                opt.allreduce_gradients()
                for p, g in zip(model.parameters(), want):
                    assert p.grad.dtype == torch.bfloat16 and _host(p.grad).ravel().tobytes() == g.tobytes(), overlap
                    raw += g.tobytes()
                assert opt.found_nonfinite is False
                assert struct.pack('<d', opt.grad_norm) == struct.pack('<d', norm), (overlap, opt.grad_norm, norm)
                raw += struct.pack('<d', opt.grad_norm)
                drop(opt)

                # the clip acts on the unscaled norm
                model, opt = make(max_grad_norm=norm / 4)
                opt.loss_scale = S
                _backward(torch, model, r, scale=S)
                opt.allreduce_gradients()
                assert struct.pack('<d', opt.grad_norm) == struct.pack('<d', norm)
                coef = (norm / 4) / (norm + 1e-6)
                for p, g in zip(model.parameters(), want):
                    clipped = torch.from_numpy(bh.wide(g).reshape(p.shape)) * coef
                    torch.testing.assert_close(p.grad.float().cpu(), clipped, rtol=2.0 ** -7, atol=0.0)  # one bf16 rounding
                drop(opt)

                model, opt = make(max_grad_norm=1e30)
                scaler = DynamicLossScaler(opt, init_scale=S, growth_interval=2)
                before = [p.detach().clone() for p in model.parameters()]
                _backward(torch, model, r, scale=scaler.scale, inject=math.inf if r == P - 1 else None)  # one rank overflows
                assert scaler.step() is False and opt.found_nonfinite and scaler.loss_scale == S / 2 == opt.loss_scale
                for p, b in zip(model.parameters(), before):
                    assert torch.equal(p.detach(), b)
                for clean in range(2):
                    _backward(torch, model, r, scale=scaler.scale)
                    assert scaler.step() is True and not opt.found_nonfinite
                    assert scaler.loss_scale == (S / 2 if clean == 0 else S)
                assert not all(torch.equal(p.detach(), b) for p, b in zip(model.parameters(), before))
                raw += b''.join(_host(p).tobytes() for p in model.parameters())
                drop(opt)
    finally:
        do.DataParallelismDistributedOptimizer._torch_sumsq = old
    _same_as_rank0(ctx, raw, 'bf16 native wrapper')


BF16_NATIVE_CHECKS = {f.__name__: f for f in (check_bf16_native_keyed_mix, check_bf16_native_wrapper)}


def worker(rank, world, port, q, only, transport):
    _mp_gpu_worker.FAULT_CHECKS.update(BF16_NATIVE_CHECKS)
    _mp_gpu_worker.worker(rank, world, port, q, only=only, transport=transport)
