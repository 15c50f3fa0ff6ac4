"""Worker of tests/test_sumsq_multiproc_gpu.py: the sum of squares of keyed allreduce results on the
whole engine over real multi-rank RCCL on one GPU. The process setup is tests/_mp_gpu_worker.worker,
unchanged; this module only adds its checks to that worker's table inside the child. Every rank
compares its doubles with the NumPy restatement over its own output and with rank 0's bits. Test
infrastructure only."""
import math
import struct

import numpy as np

import _mp_gpu_worker


def _same_as_rank0(ctx, raw, what):
    """`raw` bytes, broadcast from rank 0 as one int32 device tensor, equal this rank's."""
    torch, comm = ctx['torch'], ctx['comm']
    from ddl.torch.tensor_communicate import broadcast
    raw += b'\0' * (-len(raw) % 4)
    mine = torch.from_numpy(np.frombuffer(raw, np.int32).copy()).cuda()
    root = broadcast(mine, 0, comm)
    torch.cuda.synchronize()
    assert torch.equal(root, mine), f'{what}: bits differ from rank 0'


def plan_cuts(elements, esize, limit):
    """Where the fusion plans end inside each request (csrc/handler.cpp make_plans, restated): the
    requests, in key order, form one byte stream of `esize`-byte elements that is cut every `limit`
    bytes, a cut inside an element moving down to the element's start. Returns per request the element
    offsets (0 < offset < n) at which a new plan starts."""
    begins, total = [], 0
    for n in elements:
        begins.append(total)
        total += n * esize
    cuts = [[] for _ in elements]
    pos = 0  # bytes of the stream already planned
    while pos < total:
        end = pos + limit
        if end >= total:
            break
        i = max(q for q in range(len(elements)) if begins[q] < end and elements[q])  # (empty requests are in no plan)
        elem = (end - begins[i]) // esize
        if begins[i] + elem * esize <= pos:  # a plan makes progress: at least one element
            elem += 1
        pos = begins[i] + elem * esize
        if 0 < elem < elements[i]:
            cuts[i].append(elem)
    return cuts


def check_sumsq_keyed_mix(ctx):
    """One keyed round of an uncompressed and a bf16-compressed batch, SUM and AVG, some requests with
    the statistic and some without, every rank submitting in its own order. 256 KiB plans: the large
    requests span plans — the uncompressed one's middle plans hold it alone (the direct path, read in
    place), its first and last are fused with its neighbours (taken in the unpack)."""
    import _helpers as h
    from _sumsq_helpers import mirror
    torch, lib, comm, P, r = ctx['torch'], ctx['lib'], ctx['comm'], ctx['P'], ctx['rank']
    from ddl.torch import cpp_backend as cb
    from ddl.torch.compression import Compression
    from ddl.torch.tensor_communicate import allreduce_async_batch
    sizes = [1000, 300_000, 5, 70_001, 513, 0, 4099]
    wish = [True, True, False, True, True, True, False]
    limit = 256 << 10
    batches = {'plain': (Compression.none, cb.OP_AVG, 4), 'wire': (Compression.bf16, cb.OP_SUM, 2)}
    with h.config(lib, fusion_threshold_bytes=limit, fusion_pipeline_bytes=0):
        handles, tensors = {}, {}
        for name in (sorted(batches) if r % 2 == 0 else sorted(batches, reverse=True)):
            comp, op, _ = batches[name]
            ts = [torch.from_numpy(np.random.default_rng(31 * i + 7 * r + len(name)).standard_normal(n).astype(np.float32))
                  .cuda() for i, n in enumerate(sizes)]
            order = [int(i) for i in np.random.default_rng(5 + r).permutation(len(sizes))]
            hs = allreduce_async_batch([ts[i] for i in order], [f'sq_{name}_{i:03d}' for i in order], comm,
                                       outputs=[ts[i] for i in order], op=op, compression=comp,
                                       sumsq=[wish[i] for i in order])
            handles[name], tensors[name] = dict(zip(order, hs)), ts
        raw = b''
        for name, (comp, op, es) in sorted(batches.items()):
            cuts = plan_cuts(sizes, es, limit)  # (an empty request is in no plan and shifts nothing)
            # 4-byte elements: plans that hold the large request alone between its first and last cut
            assert len(cuts[1]) >= (3 if es == 4 else 2), cuts
            for i, n in enumerate(sizes):
                out = handles[name][i].wait(timeout=120)
                got = handles[name][i].sumsq
                assert (got is not None) == wish[i]
                if wish[i]:
                    m = mirror(out.cpu().numpy(), name == 'wire', cuts[i])
                    assert struct.pack('<d', got) == struct.pack('<d', m), (name, i, n, got, m, cuts[i])
                    raw += struct.pack('<d', got)
                raw += out.cpu().numpy().tobytes()
    _same_as_rank0(ctx, raw, 'keyed mix')


def _model(torch):
    torch.manual_seed(1234)  # the same parameters on every rank
    return torch.nn.Sequential(torch.nn.Linear(257, 300), torch.nn.Tanh(), torch.nn.Linear(300, 10)).cuda()


def _backward(torch, model, r, scale=1.0):
    g = torch.Generator().manual_seed(77 + r)  # every rank its own shard
    x = torch.randn(64, 257, generator=g).cuda()
    model.zero_grad()
    (model(x).pow(2).sum() * scale).backward()


def check_sumsq_wrapper(ctx):
    """The data-parallel wrapper with max_grad_norm, step() path and overlap_backward hooks, fused_mean
    on (the engine's quotients ARE the averaged gradients; with the default a device div_ rounds every
    element once more in fp32 and the norm of the sums over the size is no longer the norm of what
    is stored to 2^-52). grad_norm: the same bits on every rank and within n 2^-53 + 2^-52 of the fp64
    norm of the averaged gradients computed on the CPU; the clipped gradients match clip_grad_norm_ on
    a CPU copy; an injected inf is found on every rank and skip_nonfinite leaves the parameters."""
    torch, comm, P, r = ctx['torch'], ctx['comm'], ctx['P'], ctx['rank']
    from ddl.torch.parallelism.data.distributed_optimizer import data_parallelism_distributed_optimizer_wrapper as wrap
    raw = b''
    for overlap in (False, True):
        def make(**kw):
            model = _model(torch)
            opt = wrap(torch.optim.SGD(model.parameters(), lr=0.05), comm, overlap_backward=overlap, bucket_bytes=None,
                       fused_mean=True, **kw)
            return model, opt

        def drop(opt):
            for hook in getattr(opt, '_hooks', []):
                hook.remove()
        model, opt = make(max_grad_norm=1e30)  # tracked, never clipped
        _backward(torch, model, r)
        opt.allreduce_gradients()
        averaged = [p.grad.detach().cpu().clone() for p in model.parameters()]
        n = sum(g.numel() for g in averaged)
        want = math.sqrt(math.fsum(float(v) for g in averaged for v in (g.double() ** 2).flatten().tolist()))
        assert opt.found_nonfinite is False and want > 1.0
        assert abs(opt.grad_norm - want) <= (n * 2.0 ** -53 + 2.0 ** -52) * want, (overlap, opt.grad_norm, want)
        raw += struct.pack('<d', opt.grad_norm)
        drop(opt)

        limit = want / 3
        model, opt = make(max_grad_norm=limit)
        _backward(torch, model, r)
        opt.allreduce_gradients()
        assert opt.grad_norm == struct.unpack('<d', raw[-8:])[0]  # the norm before the clip, as above
        holders = [torch.nn.Parameter(torch.zeros_like(g)) for g in averaged]
        for hd, g in zip(holders, averaged):
            hd.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(holders, limit)
        for p, hd in zip(model.parameters(), holders):
            torch.testing.assert_close(p.grad.cpu(), hd.grad)
            raw += p.grad.cpu().numpy().tobytes()
        drop(opt)

        model, opt = make(skip_nonfinite=True)
        before = [p.detach().clone() for p in model.parameters()]
        _backward(torch, model, r, scale=math.inf if r == P - 1 else 1.0)  # one rank overflows
        assert opt.step() is None and opt.found_nonfinite and not math.isfinite(opt.grad_norm)
        for p, b in zip(model.parameters(), before):
            assert torch.equal(p.detach(), b)
        _backward(torch, model, r)
        opt.step()
        assert not opt.found_nonfinite
        assert not all(torch.equal(p.detach(), b) for p, b in zip(model.parameters(), before))
        drop(opt)
    _same_as_rank0(ctx, raw, 'wrapper')


SUMSQ_CHECKS = {f.__name__: f for f in (check_sumsq_keyed_mix, check_sumsq_wrapper)}


def worker(rank, world, port, q, only):
    _mp_gpu_worker.FAULT_CHECKS.update(SUMSQ_CHECKS)
    _mp_gpu_worker.worker(rank, world, port, q, only=only, transport='rccl')
