"""Worker of tests/test_wire_multiproc_gpu.py: wire compression (ddl_allreduce_wire) on the whole
engine over real multi-rank RCCL on one GPU. The process setup is tests/_mp_gpu_worker.worker,
unchanged; this module only adds its checks to that worker's table inside the child. Expected
values are _wire_helpers.expected: the CPU's casts of every rank's input, the oracle's sum of them
in MPICH's order for the plan's wire bytes, widened and divided on the CPU. Test infrastructure only."""
import numpy as np

import _mp_gpu_worker


def check_wire_keyed_batch(ctx):
    """A keyed batch of 6 fp32 device tensors, one fp16 device tensor and one CPU tensor through
    allreduce_async_batch(compression=Compression.fp16), every rank submitting in its own order: the
    fp32 device tensors form ONE compressed plan (cut into 64 KiB sub-plans of the wire stream)
    and equal the contract's value; the fp16 and the CPU tensor are reduced as without the flag
    and equal the plain oracle sums."""
    import _avg_helpers as a
    import _helpers as h
    import _wire_helpers as w
    torch, lib, comm, P, r, ora = ctx['torch'], ctx['lib'], ctx['comm'], ctx['P'], ctx['rank'], ctx['oracle']
    from ddl.torch import Compression
    from ddl.torch.tensor_communicate import allreduce_async_batch
    elems = [5, 300, 70_001, 4099, 1, 513]
    xs = [[w.wire_input(n, 7000 + 31 * q + i) for i, n in enumerate(elems)] for q in range(P)]
    hs16 = [h.random_input(h.DT_HALF, 4099, 7100 + q) for q in range(P)]
    cpu32 = [h.random_input(h.DT_FLOAT, 3001, 7200 + q) for q in range(P)]
    ts = [torch.from_numpy(x).cuda() for x in xs[r]] + [torch.from_numpy(hs16[r]).cuda(), torch.from_numpy(cpu32[r])]
    names = [f'wire_{i:03d}' for i in range(len(ts))]
    order = [int(i) for i in np.random.default_rng(90 + r).permutation(len(ts))]
    with h.config(lib, fusion_pipeline_bytes=64 << 10):
        handles = allreduce_async_batch([ts[i] for i in order], [names[i] for i in order], comm,
                                        compression=Compression.fp16)
        assert [hd.key for hd in handles] == [names[i] for i in order]  # the caller's order
        got = {i: hd.wait(timeout=120) for i, hd in zip(order, handles)}
    message = 2 * sum(elems)  # the compressed plan's unpadded wire bytes
    for i, n in enumerate(elems):
        assert got[i].dtype == torch.float32 and got[i].is_cuda
        want = w.expected(ora, h.DT_HALF, [xs[q][i] for q in range(P)], message, w.OP_SUM, P)
        a.assert_same(h.DT_FLOAT, got[i].cpu().numpy(), want, f'fp32 over fp16, tensor {i} ({n} elements)')
    a.assert_same(h.DT_HALF, got[6].cpu().numpy(), ora.fold_ref_order(h.DT_HALF, hs16), 'the fp16 tensor')
    assert not got[7].is_cuda
    a.assert_same(h.DT_FLOAT, got[7].numpy(), ora.fold_ref_order(h.DT_FLOAT, cpu32), 'the CPU tensor')


def check_wire_dp_wrapper(ctx):
    """One step of the DP wrapper on a 3-layer fp32 MLP with compression=Compression.bf16 and
    fused_mean=True: every parameter's gradient after the step is the contract's value computed from
    the ranks' own gradients (exchanged over the test's gloo group): bf16 casts, the oracle's sum
    for the one plan's wire bytes, widened, divided by np.float32(P). No div_ runs."""
    import _avg_helpers as a
    import _helpers as h
    import _wire_helpers as w
    from _mp_avg_worker import _count_div
    torch, comm, P, r, ora, dist = ctx['torch'], ctx['comm'], ctx['P'], ctx['rank'], ctx['oracle'], ctx['dist']
    from ddl.torch import Compression
    from ddl.torch.parallelism.data import data_parallelism_distributed_optimizer_wrapper
    torch.manual_seed(4321)  # the same weights on every rank
    model = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.Tanh(), torch.nn.Linear(32, 32), torch.nn.Tanh(),
                                torch.nn.Linear(32, 4)).cuda()
    opt = data_parallelism_distributed_optimizer_wrapper(torch.optim.SGD(model.parameters(), lr=0.1), comm,
                                                         compression=Compression.bf16, fused_mean=True)
    g = torch.Generator().manual_seed(55 + r)  # its own shard of the batch
    x, y = torch.randn(8, 16, generator=g).cuda(), torch.randn(8, 4, generator=g).cuda()
    torch.nn.functional.mse_loss(model(x), y).backward()
    params = list(model.parameters())
    mine = [p.grad.detach().cpu().contiguous() for p in params]
    theirs = []  # theirs[i][q]: rank q's gradient of parameter i
    for t in mine:
        parts = [torch.empty_like(t) for _ in range(P)]
        dist.all_gather(parts, t)
        theirs.append([p.numpy().reshape(-1) for p in parts])
    with _count_div(torch) as divs:
        opt.step()
    assert not divs, divs
    message = 2 * sum(p.numel() for p in params)  # one fp32-over-bf16 plan, keys in parameter order
    for i, p in enumerate(params):
        want = w.expected(ora, h.DT_BFLOAT16, theirs[i], message, w.OP_AVG, P)
        a.assert_same(h.DT_FLOAT, p.grad.detach().cpu().numpy().reshape(-1), want, f'parameter {i}')


WIRE_CHECKS = {f.__name__: f for f in (check_wire_keyed_batch, check_wire_dp_wrapper)}


def worker(rank, world, port, q, only):
    _mp_gpu_worker.FAULT_CHECKS.update(WIRE_CHECKS)
    _mp_gpu_worker.worker(rank, world, port, q, only=only, transport='rccl')
