"""Worker of tests/test_avg_multiproc_gpu.py: the AVG op (DDL_ALLREDUCE_OP_AVG) on the whole engine
over real multi-rank RCCL on one GPU. The process setup is tests/_mp_gpu_worker.worker, unchanged;
this module only adds its checks to that worker's table inside the child. Expected values are
exact integer sums, or the oracle's sum in MPICH's order, divided on the CPU
(_avg_helpers.quotient). Test infrastructure only."""
import contextlib

import numpy as np

import _mp_gpu_worker


def _bits(t):
    """A tensor's bytes as numpy (any dtype, bf16 included)."""
    import torch
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()


def _cpu_mean(torch, total, P):
    """torch CPU's quotient of an exact sum: the AVG contract's value (IEEE; bf16 / fp16 through fp32)."""
    return total.cpu().div(P)


def check_avg_keyed_mix(ctx):
    """One SUM batch and one AVG batch in the same keyed round, keys interleaved (so SUM and AVG
    requests share dtype groups, plans capped at 1 MiB + 1, sub-plans and unpack launches), every
    rank submitting in its own order: device fp32 / fp64 / fp16 / bf16, pinned host fp64 (its plans
    are unpacked by the dividing kernel straight into the outputs), host fp32 pinned and pageable
    (staged: divided in the device slot). Integer-valued data: every sum is exact, SUM results are
    the sums, AVG results their CPU quotients, bit for bit."""
    import _helpers as h
    torch, lib, comm, P, r = ctx['torch'], ctx['lib'], ctx['comm'], ctx['P'], ctx['rank']
    from ddl.torch import cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async_batch
    kinds = [('cuda', torch.float32), ('cuda', torch.float64), ('cuda', torch.float16), ('cuda', torch.bfloat16),
             ('pinned', torch.float64), ('pinned', torch.float32), ('host', torch.float32)]
    rng = np.random.default_rng(23)
    k = 42  # 21 per batch
    sizes = [int(np.exp(rng.uniform(0, np.log(200_000)))) for _ in range(k)]
    sizes[5], sizes[12] = 200_000, 70_001
    with h.config(lib, fusion_threshold_bytes=(1 << 20) + 1, fusion_pipeline_bytes=256 << 10, host_chunk_bytes=64 << 10):
        base = [torch.randint(-8, 9, (sizes[i],), generator=torch.Generator().manual_seed(300 + i)) for i in range(k)]
        ts, want = [], []
        for i in range(k):
            where, dt = kinds[(i // 2) % len(kinds)]  # both batches get every kind
            t = (base[i] + r).to(dt)
            t = t.cuda() if where == 'cuda' else t.pin_memory() if where == 'pinned' else t
            ts.append(t)
            total = (base[i] * P + P * (P - 1) // 2).to(dt)
            want.append(total if i % 2 == 0 else _cpu_mean(torch, total, P))
        plans0 = lib.ddl_get_config(b'host_zero_copy_plans')
        handles = {}
        batches = [(0, cb.OP_SUM), (1, cb.OP_AVG)]
        for parity, op in (batches if r % 2 == 0 else batches[::-1]):
            order = [int(i) for i in np.random.default_rng(50 + 7 * r + parity).permutation(k) if i % 2 == parity]
            outs = [ts[i] if not ts[i].is_cuda else torch.empty_like(ts[i]) for i in order]  # host in place
            hs = allreduce_async_batch([ts[i] for i in order], [f'mix_{i:04d}' for i in order], comm, outputs=outs, op=op)
            handles.update(dict(zip(order, hs)))
        for i in range(k):
            got = handles[i].wait(timeout=120)
            assert _bits(got) == _bits(want[i]), (i, kinds[(i // 2) % len(kinds)], sizes[i], 'avg' if i % 2 else 'sum')
        assert lib.ddl_get_config(b'host_zero_copy_plans') > plans0  # the pinned fp64 group


def check_avg_direct(ctx):
    """The unfused entry points with AVG: allreduce of a device tensor and of a CPU tensor (the
    chunked host pipeline, many chunks: divided per device chunk), and the grouped allreduce_batch_."""
    import _avg_helpers as a
    import _helpers as h
    torch, lib, comm, P, r, ora = ctx['torch'], ctx['lib'], ctx['comm'], ctx['P'], ctx['rank'], ctx['oracle']
    from ddl.torch import cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce, allreduce_, allreduce_batch_
    for dt, n in ((h.DT_FLOAT, 300_001), (h.DT_DOUBLE, 4099), (h.DT_FLOAT, 7)):
        xs = [h.random_input(dt, n, 610 + 13 * q + n) for q in range(P)]
        want = a.quotient(dt, ora.fold_ref_order(dt, xs), P)
        t = torch.from_numpy(xs[r]).cuda()
        a.assert_same(dt, allreduce(t, comm, op=cb.OP_AVG).cpu().numpy(), want, f'allreduce n={n}')
        a.assert_same(dt, allreduce_(t, comm, op=cb.OP_AVG).cpu().numpy(), want, f'allreduce_ n={n}')
    n = 1_000_003
    base = torch.randint(-1000, 1000, (n,), generator=torch.Generator().manual_seed(9))
    with h.config(lib, host_chunk_bytes=256 << 10):
        got = allreduce((base + r).to(torch.float32), comm, op=cb.OP_AVG)
    assert not got.is_cuda
    assert torch.equal(got, (base * P + P * (P - 1) // 2).to(torch.float32).div(P))
    ns = [300, 0, 4099, 65_537, 1]
    for dt in (h.DT_FLOAT, h.DT_HALF):
        xs = [[h.random_input(dt, m, 2000 * q + 17 * b + dt) for b, m in enumerate(ns)] for q in range(P)]
        ts = [torch.from_numpy(x).cuda() for x in xs[r]]
        allreduce_batch_(ts, comm, op=cb.OP_AVG)
        torch.cuda.synchronize()
        for b, m in enumerate(ns):
            if m:
                want = a.quotient(dt, ora.fold_ref_order(dt, [xs[q][b] for q in range(P)]), P)
                a.assert_same(dt, ts[b].cpu().numpy(), want, f'batch bucket {b}')


@contextlib.contextmanager
def _count_div(torch):
    calls, real = [], torch.Tensor.div_

    def counting(self, *args, **kw):
        calls.append(args)
        return real(self, *args, **kw)
    torch.Tensor.div_ = counting
    try:
        yield calls
    finally:
        torch.Tensor.div_ = real


def check_avg_dp_wrapper(ctx):
    """The DP wrapper with fused_mean=True on the models of check_dp_training (GPU) and
    check_dp_training_cpu_model (CPU, pinned gradients), overlap_backward off and on: three steps
    equal the full-batch fp64 steps, the wrapper's steps call no Tensor.div_, and the CPU model's
    parameters equal, bit for bit, a second replica's trained with fused_mean=False (both sides
    divide by IEEE: torch CPU's div_ and the engine's kernel)."""
    import _helpers as h
    torch, lib, comm, P, r = ctx['torch'], ctx['lib'], ctx['comm'], ctx['P'], ctx['rank']
    from ddl.torch.parallelism.data import InitialParametersBroadcast, data_parallelism_distributed_optimizer_wrapper
    F = torch.nn.functional
    for dev, seed in (('cuda', 1234), ('cpu', 99)):
        for overlap in (False, True):
            def model_fn(s):
                torch.manual_seed(s)
                return torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.Tanh(), torch.nn.Linear(32, 4)).double().to(dev)
            model, twin, ref = model_fn(seed + r), model_fn(seed + r), model_fn(seed)
            for m in (model, twin):
                InitialParametersBroadcast(m, 0, communicator=comm).broadcast()
            with h.config(lib, fusion_threshold_bytes=lib.ddl_get_config(b'fusion_threshold_bytes')):  # restored
                opt = data_parallelism_distributed_optimizer_wrapper(torch.optim.SGD(model.parameters(), lr=0.1), comm,
                                                                     overlap_backward=overlap, fused_mean=True)
                topt = data_parallelism_distributed_optimizer_wrapper(torch.optim.SGD(twin.parameters(), lr=0.1), comm,
                                                                      overlap_backward=overlap)
                ref_opt = torch.optim.SGD(ref.parameters(), lr=0.1)
                g = torch.Generator().manual_seed(77)
                for step in range(3):
                    xb = [torch.randn(8, 16, generator=g, dtype=torch.float64).to(dev) for _ in range(P)]
                    yb = [torch.randn(8, 4, generator=g, dtype=torch.float64).to(dev) for _ in range(P)]
                    opt.zero_grad()
                    F.mse_loss(model(xb[r]), yb[r]).backward()
                    if overlap:
                        assert len(opt._grad_handles) == len(list(model.parameters()))
                    with _count_div(torch) as divs:
                        opt.step()
                    assert not divs, divs
                    topt.zero_grad()
                    F.mse_loss(twin(xb[r]), yb[r]).backward()
                    topt.step()
                    ref_opt.zero_grad()
                    sum(F.mse_loss(ref(xb[q]), yb[q]) for q in range(P)).div(P).backward()
                    ref_opt.step()
            for p, t, q in zip(model.parameters(), twin.parameters(), ref.parameters()):
                assert torch.allclose(p, q, rtol=1e-12, atol=1e-12), (dev, overlap)
                if dev == 'cpu':
                    assert torch.equal(p, t), (dev, overlap)


AVG_CHECKS = {f.__name__: f for f in (check_avg_keyed_mix, check_avg_direct, check_avg_dp_wrapper)}


def worker(rank, world, port, q, only):
    _mp_gpu_worker.FAULT_CHECKS.update(AVG_CHECKS)
    _mp_gpu_worker.worker(rank, world, port, q, only=only, transport='rccl')
