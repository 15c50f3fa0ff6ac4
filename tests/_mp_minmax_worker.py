"""Worker of tests/test_minmax_multiproc_gpu.py: DDL_ALLREDUCE_OP_MIN / _MAX on the whole engine over
real multi-rank RCCL on one GPU. The process setup is tests/_mp_gpu_worker.worker, unchanged; this
module only adds its checks to that worker's table inside the child. Every rank builds every rank's
inputs from the seeds, so expected values are the numpy model's (_minmax_helpers.model; sums are
exact integer sums); and every rank compares its result bits with rank 0's. Test infrastructure
only."""
import numpy as np

import _mp_gpu_worker


def _bits(t):
    import torch
    if t.numel() == 0:
        return b''
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()


def _same_as_rank0(ctx, tensors, what):
    """Every result's bytes, broadcast from rank 0 as one int32 device tensor, equal this rank's."""
    torch, comm = ctx['torch'], ctx['comm']
    from ddl.torch.tensor_communicate import broadcast
    raw = b''.join(_bits(t) for t in tensors)
    raw += b'\0' * (-len(raw) % 4)
    mine = torch.from_numpy(np.frombuffer(raw, np.int32).copy()).cuda()
    root = broadcast(mine, 0, comm)
    torch.cuda.synchronize()
    assert torch.equal(root, mine), f'{what}: bits differ from rank 0'


NP_OF = {'float32': np.float32, 'float16': np.float16, 'int32': np.int32}


def check_minmax_keyed_mix(ctx):
    """One keyed round of four batches — SUM, AVG, MIN, MAX — with keys interleaved, fp32 / fp16 /
    int32 (AVG: the float types) on device, pinned and pageable tensors, every rank submitting in its
    own order; the fusion threshold leaves fused plans and single-request plans, the pipeline cut
    sub-plans. Integer-valued data: sums are exact, MIN / MAX are the model's."""
    import _helpers as h
    import _minmax_helpers as mm
    torch, lib, comm, P, r = ctx['torch'], ctx['lib'], ctx['comm'], ctx['P'], ctx['rank']
    from ddl.torch import cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async_batch
    DT = {'float32': h.DT_FLOAT, 'float16': h.DT_HALF, 'int32': h.DT_INT32}
    kinds = [(w, d) for w in ('cuda', 'pinned', 'host') for d in ('float32', 'float16', 'int32')]
    ops = [cb.OP_SUM, cb.OP_AVG, cb.OP_MIN, cb.OP_MAX]
    rng = np.random.default_rng(29)
    k = 72  # 18 per op: every (memory, dtype) twice
    sizes = [int(np.exp(rng.uniform(0, np.log(100_000)))) for _ in range(k)]
    sizes[6], sizes[11], sizes[3] = 400_000, 70_001, 300_000  # above the threshold: plans of their own
    with h.config(lib, fusion_threshold_bytes=(1 << 20) + 1, fusion_pipeline_bytes=256 << 10, host_chunk_bytes=64 << 10):
        ts, want = [], []
        for i in range(k):
            op = ops[i % 4]
            where, d = kinds[(i // 4) % len(kinds)]
            if op == cb.OP_AVG and d == 'int32':
                d = 'float32'
            xs = [np.random.default_rng(1000 * i + q).integers(-8, 9, sizes[i]).astype(NP_OF[d]) for q in range(P)]
            if op in (cb.OP_MIN, cb.OP_MAX):
                w = mm.model(DT[d], op, xs)
            else:
                w = np.sum(np.stack([x.astype(np.float64) for x in xs]), axis=0)  # exact
                w = (w.astype(np.float32) / np.float32(P) if op == cb.OP_AVG else w).astype(NP_OF[d])
            t = torch.from_numpy(xs[r])
            ts.append(t.cuda() if where == 'cuda' else t.pin_memory() if where == 'pinned' else t)
            want.append(w)
        handles = {}
        batches = list(enumerate(ops))
        for j, op in (batches if r % 2 == 0 else batches[::-1]):
            order = [int(i) for i in np.random.default_rng(50 + 7 * r + j).permutation(k) if i % 4 == j]
            outs = [ts[i] if not ts[i].is_cuda else torch.empty_like(ts[i]) for i in order]  # host in place
            hs = allreduce_async_batch([ts[i] for i in order], [f'mm_{i:04d}' for i in order], comm, outputs=outs, op=op)
            handles.update(dict(zip(order, hs)))
        got = [handles[i].wait(timeout=120) for i in range(k)]
        for i in range(k):
            assert _bits(got[i]) == want[i].tobytes(), (i, ops[i % 4], kinds[(i // 4) % len(kinds)], sizes[i])
    _same_as_rank0(ctx, got, 'keyed mix')


def check_minmax_direct(ctx):
    """allreduce / allreduce_ of device tensors of every dtype the torch side has, a CPU tensor
    through the chunked host pipeline, and the grouped allreduce_batch_, with MIN and MAX."""
    import _helpers as h
    import _minmax_helpers as mm
    torch, lib, comm, P, r = ctx['torch'], ctx['lib'], ctx['comm'], ctx['P'], ctx['rank']
    from ddl.torch import cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce, allreduce_, allreduce_batch_
    results = []
    for op in (cb.OP_MIN, cb.OP_MAX):
        for dt, n in ((h.DT_FLOAT, 300_001), (h.DT_DOUBLE, 4099), (h.DT_FLOAT, 7), (h.DT_HALF, 70_001),
                      (h.DT_INT32, 4099), (h.DT_INT64, 513)):
            xs = [mm.finite_input(dt, n, 610 + 13 * q + n) for q in range(P)]
            want = mm.model(dt, op, xs)
            t = torch.from_numpy(xs[r]).cuda()
            out = allreduce(t, comm, op=op)
            mm.assert_same(dt, out.cpu().numpy(), want, f'allreduce op={op} n={n}')
            mm.assert_same(dt, allreduce_(t, comm, op=op).cpu().numpy(), want, f'allreduce_ op={op} n={n}')
            results.append(out)
        # a NaN on one rank reaches every rank; -0 against +0 is ordered
        x = torch.tensor([1.0, 0.0 if r else -0.0, float(r)], device='cuda')
        if r == P - 1:
            x[0] = float('nan')
        y = allreduce(x, comm, op=op).cpu()
        assert torch.isnan(y[0]) and bool(torch.signbit(y[1])) == (op == cb.OP_MIN), y
        assert y[2].item() == (P - 1 if op == cb.OP_MAX else 0)
        n = 1_000_003
        xs = [mm.finite_input(h.DT_FLOAT, n, 9 + q) for q in range(P)]
        with h.config(lib, host_chunk_bytes=256 << 10):
            got = allreduce(torch.from_numpy(xs[r]), comm, op=op)
        assert not got.is_cuda
        mm.assert_same(h.DT_FLOAT, got.numpy(), mm.model(h.DT_FLOAT, op, xs), f'host allreduce op={op}')
        results.append(got)
        ns = [300, 0, 4099, 65_537, 1]
        for dt in (h.DT_FLOAT, h.DT_HALF, h.DT_INT32):
            xs = [[mm.finite_input(dt, m, 2000 * q + 17 * b + dt) for b, m in enumerate(ns)] for q in range(P)]
            ts = [torch.from_numpy(x).cuda() for x in xs[r]]
            allreduce_batch_(ts, comm, op=op)
            torch.cuda.synchronize()
            for b, m in enumerate(ns):
                mm.assert_same(dt, ts[b].cpu().numpy(), mm.model(dt, op, [xs[q][b] for q in range(P)]), f'bucket {b}')
            results += ts
    _same_as_rank0(ctx, results, 'direct')


def check_minmax_metrics(ctx):
    """MetricAverage(ops=...): the named metrics take their op, the others are averaged as ever."""
    torch, comm, P, r = ctx['torch'], ctx['comm'], ctx['P'], ctx['rank']
    from ddl.torch import cpp_backend as cb
    from ddl.torch.parallelism.data import MetricAverage
    logs = {'loss': 1.0 + r, 'best': 10.0 - r, 'step_time': 0.5 * (r + 1), 'seen': 3.0, 'acc': 0.25 * r}
    cbk = MetricAverage(comm, ops={'best': cb.OP_MIN, 'step_time': cb.OP_MAX, 'seen': cb.OP_SUM})
    out = cbk.on_epoch_end(0, dict(logs))
    assert out == {'loss': sum(1.0 + q for q in range(P)) / P, 'best': 10.0 - (P - 1), 'step_time': 0.5 * P,
                   'seen': 3.0 * P, 'acc': sum(0.25 * q for q in range(P)) / P}, out
    plain = MetricAverage(comm).on_epoch_end(0, dict(logs))
    assert plain == {k: sum(v for v in vs) / P for k, vs in
                     {'loss': [1.0 + q for q in range(P)], 'best': [10.0 - q for q in range(P)],
                      'step_time': [0.5 * (q + 1) for q in range(P)], 'seen': [3.0] * P,
                      'acc': [0.25 * q for q in range(P)]}.items()}, plain


MINMAX_CHECKS = {f.__name__: f for f in (check_minmax_keyed_mix, check_minmax_direct, check_minmax_metrics)}


def worker(rank, world, port, q, only):
    _mp_gpu_worker.FAULT_CHECKS.update(MINMAX_CHECKS)
    _mp_gpu_worker.worker(rank, world, port, q, only=only, transport='rccl')
