"""Worker of tests/test_scale_multiproc_gpu.py: the scale factors of keyed allreduces on the whole engine
in several processes on one GPU. The process setup is tests/_mp_gpu_worker.worker, unchanged; this module
only adds its checks to that worker's table inside the child. The model: the engine's own UNSCALED
requests (SUM) on NumPy-prescaled inputs give the reduced stream, NumPy takes the quotient and the
postscale; every rank also compares its bits with rank 0's. Test infrastructure only."""
import math
import struct

import numpy as np

import _mp_gpu_worker
from _mp_sumsq_worker import _same_as_rank0, plan_cuts

SIZES = [1000, 300_000, 5, 70_001, 513, 0, 4099]


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _same_double(a, b):
    return (math.isnan(a) and math.isnan(b)) or struct.pack('<d', a) == struct.pack('<d', b)


def check_scale_keyed_mix(ctx):
    """Keyed batches that mix scaled and unscaled requests, AVG and SUM batches, without a wire and over bf16, with
    sums of squares; 256 KiB plans, so the large requests span plans (fused, and alone in the middle: the
    direct path with its in-place postscale, or the fusion-buffer path where they carry a prescale)."""
    import _helpers as h
    from _scale_helpers import mixed_factors, mul, result, same_bits, scale_input
    from _sumsq_helpers import mirror
    torch, lib, comm, P, r = ctx['torch'], ctx['lib'], ctx['comm'], ctx['P'], ctx['rank']
    from ddl.torch import cpp_backend as cb
    from ddl.torch.compression import Compression
    from ddl.torch.tensor_communicate import allreduce_async_batch
    k = len(SIZES)
    limit = 256 << 10
    raw = b''
    with h.config(lib, fusion_threshold_bytes=limit, fusion_pipeline_bytes=0):
        for name, comp, es, shift in (('plain', Compression.none, 4, 0), ('wire', Compression.bf16, 2, 1),
                                      ('post', Compression.none, 4, 3)):
            pre, post = mixed_factors(k, shift), mixed_factors(k, shift + 2)
            if name == 'post':  # no prescale anywhere: the large request's middle plans take the direct path
                pre = [np.float32(1)] * k
            op = cb.OP_SUM if name == 'wire' else cb.OP_AVG  # (one op per batch; SUM and AVG across the batches)
            ops = [op] * k
            xs = [scale_input(n, 31 * i + 7 * r + shift, pre[i]) for i, n in enumerate(SIZES)]
            # the reduced stream: the engine's unscaled SUM of the prescaled inputs, in a round cut alike
            ref = [_dev(torch, mul(x, a)) for x, a in zip(xs, pre)]
            hs = allreduce_async_batch(ref, [f'scm_{name}_ref_{i:03d}' for i in range(k)], comm, outputs=ref,
                                       op=cb.OP_SUM, compression=comp)
            sums = [hh.wait(timeout=120).cpu().numpy() for hh in hs]
            ts = [_dev(torch, x) for x in xs]
            order = [int(i) for i in np.random.default_rng(5 + r).permutation(k)]  # every rank in its own order
            wish = [i % 3 != 2 for i in range(k)]
            got = allreduce_async_batch([ts[i] for i in order], [f'scm_{name}_{i:03d}' for i in order], comm,
                                        outputs=[ts[i] for i in order], op=op, compression=comp,
                                        prescale=[float(pre[i]) for i in order], postscale=[float(post[i]) for i in order],
                                        sumsq=[wish[i] for i in order])
            handles = dict(zip(order, got))
            outs = {i: handles[i].wait(timeout=120).cpu().numpy() for i in range(k)}
            for i in range(k):
                model = result(sums[i], ops[i], P, post[i])
                assert same_bits(outs[i], model), (name, i, SIZES[i], float(pre[i]), float(post[i]), ops[i])
                raw += np.where(np.isnan(outs[i]), np.float32(0), outs[i]).tobytes() + np.isnan(outs[i]).tobytes()
            # the sums of squares on finite data (bits), in a round of their own with the same cuts
            ys = [np.random.default_rng(100 + 13 * i + r).standard_normal(n).astype(np.float32) for i, n in enumerate(SIZES)]
            ts = [_dev(torch, y) for y in ys]
            hs = allreduce_async_batch(ts, [f'scm_{name}_sq_{i:03d}' for i in range(k)], comm, outputs=ts, op=cb.OP_AVG,
                                       compression=comp, prescale=[float(a) for a in pre], postscale=[float(b) for b in post],
                                       sumsq=True)
            cuts = plan_cuts(SIZES, es, limit)
            assert len(cuts[1]) >= 2, cuts
            for i, hh in enumerate(hs):
                out = hh.wait(timeout=120).cpu().numpy()
                m = mirror(out, name == 'wire', cuts[i])
                assert math.isfinite(m) and _same_double(hh.sumsq, m), (name, i, hh.sumsq, m, cuts[i])
                raw += struct.pack('<d', hh.sumsq)
    _same_as_rank0(ctx, raw, 'scaled keyed mix')


def check_scale_disagree(ctx):
    """The ranks pass DIFFERENT factors (rank-local, like the op): rank 0 no prescale at all, the others 0.5,
    and every rank a postscale of its own. The round completes on every rank — the large request's middle
    plans hold it alone, where a rank with a prescale and a rank without must post the same collective —
    and every rank gets its own postscale applied to the common sum of the ranks' own prescaled inputs."""
    import _helpers as h
    from _scale_helpers import FACTORS, mul, result, same_bits
    torch, lib, comm, P, r = ctx['torch'], ctx['lib'], ctx['comm'], ctx['P'], ctx['rank']
    from ddl.torch import cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async_batch
    sizes = [70_001, 5, 300_000]
    b = FACTORS[(r + 1) % len(FACTORS)]  # rank 0: 0.5, rank 1: 1/3, rank 2: 3
    mine = [b, np.float32(1) if r == 0 else b, b]  # on rank 0 the second request is not scaled at all
    with h.config(lib, fusion_threshold_bytes=256 << 10, fusion_pipeline_bytes=0):
        xs = [np.random.default_rng(17 * i + r).standard_normal(n).astype(np.float32) for i, n in enumerate(sizes)]
        a = np.float32(1) if r == 0 else np.float32(0.5)
        ref = [_dev(torch, mul(x, a)) for x in xs]
        hs = allreduce_async_batch(ref, [f'scd_ref_{i}' for i in range(3)], comm, outputs=ref, op=cb.OP_SUM)
        sums = [hh.wait(timeout=120).cpu().numpy() for hh in hs]
        ts = [_dev(torch, x) for x in xs]
        hs = allreduce_async_batch(ts, [f'scd_{i}' for i in range(3)], comm, outputs=ts, op=cb.OP_AVG,
                                   prescale=float(a), postscale=[float(v) for v in mine])
        for i, hh in enumerate(hs):
            out = hh.wait(timeout=120).cpu().numpy()
            assert same_bits(out, result(sums[i], cb.OP_AVG, P, mine[i])), (i, float(mine[i]))
    _same_as_rank0(ctx, b''.join(s.tobytes() for s in sums), 'the common sums')


def _model(torch):
    torch.manual_seed(1234)  # the same parameters on every rank
    return torch.nn.Sequential(torch.nn.Linear(257, 300), torch.nn.Tanh(), torch.nn.Linear(300, 10)).cuda()


def _backward(torch, model, r, scale=1.0, inject=None):
    g = torch.Generator().manual_seed(77 + r)  # every rank its own shard
    x = torch.randn(64, 257, generator=g).cuda()
    model.zero_grad()
    loss = model(x).pow(2).sum()
    if inject is not None:
        loss = loss * inject
    (loss * scale if not callable(scale) else scale(loss)).backward()


def check_scale_wrapper(ctx):
    """The data-parallel wrapper with fused_mean, gradient_predivide_factor = 2, loss_scale = 1024 and
    max_grad_norm set, on the step() path and the overlap_backward hooks. The gradients are a plain
    wrapper's over the same scaled gradients halved by torch (exact), followed by NumPy's product with
    float32(2 / 1024); grad_norm is sqrt(fsum(mirror(g))) of those unscaled gradients; a step with an
    injected inf is skipped and DynamicLossScaler halves its scale, and doubles it after two clean steps."""
    import _helpers as h
    from _scale_helpers import mul
    from _sumsq_helpers import mirror
    torch, lib, comm, P, r = ctx['torch'], ctx['lib'], ctx['comm'], ctx['P'], ctx['rank']
    from ddl.torch.parallelism.data import DynamicLossScaler
    from ddl.torch.parallelism.data.distributed_optimizer import data_parallelism_distributed_optimizer_wrapper as wrap
    S, f = 1024.0, 2.0
    raw = b''
    with h.config(lib, fusion_pipeline_bytes=0):
        for overlap in (False, True):
            def make(**kw):
                model = _model(torch)
                opt = wrap(torch.optim.SGD(model.parameters(), lr=0.05), comm, overlap_backward=overlap, bucket_bytes=None,
                           fused_mean=True, **kw)
                return model, opt

            def drop(opt):
                for hook in getattr(opt, '_hooks', []):
                    hook.remove()
            # the plain wrapper (no hooks: the gradients are halved before they are submitted)
            model = _model(torch)
            plain = wrap(torch.optim.SGD(model.parameters(), lr=0.05), comm, fused_mean=True)
            _backward(torch, model, r, scale=S)
            for p in model.parameters():
                p.grad.mul_(1.0 / f)
            plain.allreduce_gradients()
            want = [mul(p.grad.cpu().numpy(), np.float32(f * (1.0 / S))) for p in model.parameters()]
            norm = math.sqrt(math.fsum(mirror(g, False) for g in want))
            assert math.isfinite(norm) and norm > 1.0

            model, opt = make(gradient_predivide_factor=f, max_grad_norm=1e30)
            opt.loss_scale = S
            _backward(torch, model, r, scale=S)
            opt.allreduce_gradients()
            for p, g in zip(model.parameters(), want):
                assert p.grad.cpu().numpy().tobytes() == g.tobytes(), overlap
                raw += g.tobytes()
            assert opt.found_nonfinite is False
            assert struct.pack('<d', opt.grad_norm) == struct.pack('<d', norm), (overlap, opt.grad_norm, norm)
            drop(opt)

            # the clip acts on the unscaled norm
            model, opt = make(gradient_predivide_factor=f, max_grad_norm=norm / 4)
            opt.loss_scale = S
            _backward(torch, model, r, scale=S)
            opt.allreduce_gradients()
            coef = (norm / 4) / (norm + 1e-6)
            for p, g in zip(model.parameters(), want):
                torch.testing.assert_close(p.grad.cpu(), torch.from_numpy(g) * coef)
            drop(opt)

            model, opt = make(gradient_predivide_factor=f, max_grad_norm=1e30)
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
            raw += b''.join(p.detach().cpu().numpy().tobytes() for p in model.parameters())
            drop(opt)
    _same_as_rank0(ctx, raw, 'scaled wrapper')


SCALE_CHECKS = {f.__name__: f for f in (check_scale_keyed_mix, check_scale_disagree, check_scale_wrapper)}


def worker(rank, world, port, q, only, transport):
    _mp_gpu_worker.FAULT_CHECKS.update(SCALE_CHECKS)
    _mp_gpu_worker.worker(rank, world, port, q, only=only, transport=transport)
