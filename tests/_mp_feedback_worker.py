"""Worker of tests/test_feedback_multiproc_gpu.py: error feedback of the 16-bit wire
(DDL_ALLREDUCE_WIRE_FEEDBACK) on the whole engine over real multi-rank RCCL on one GPU. The process
setup is tests/_mp_gpu_worker.worker, unchanged; this module only adds its checks to that worker's
table inside the child. Every rank runs the CPU model (_feedback_helpers) for ALL ranks' inputs —
their wire values and residuals round after round — and compares its own results with the oracle's
sum of the wire values, widened and divided on the CPU. Test infrastructure only."""
import numpy as np

import _mp_gpu_worker

ROUNDS = 3


def check_feedback_keyed_batch(ctx):
    """Three rounds under the same keys: two fp32 device tensors with bf16 feedback and a native
    fp16 tensor in one batch, and an fp32 tensor over the plain bf16 wire submitted next to it. Every
    compressed tensor is more than 2048 wire bytes and P <= 3, so MPICH's order is the same whichever
    way the two submissions share rounds and plans. The 70_001-element tensor is cut across 64 KiB
    sub-plans."""
    import _avg_helpers as a
    import _feedback_helpers as f
    import _helpers as h
    import _wire_helpers as w
    torch, lib, comm, P, r, ora = ctx['torch'], ctx['lib'], ctx['comm'], ctx['P'], ctx['rank'], ctx['oracle']
    from ddl.torch import Compression
    from ddl.torch.tensor_communicate import allreduce_async, allreduce_async_batch
    wire, fb_elems, plain_elems, message = h.DT_BFLOAT16, [70_001, 4099], 3001, 1 << 20
    names = ['fbmp_a', 'fbmp_b', 'fbmp_half']
    resid = [[np.zeros(n, np.float32) for n in fb_elems] for _ in range(P)]
    for t in range(ROUNDS):
        xs = [[w.wire_input(n, 9000 + 500 * t + 31 * q + i) for i, n in enumerate(fb_elems)] for q in range(P)]
        plain = [w.wire_input(plain_elems, 9300 + 500 * t + q) for q in range(P)]
        hs16 = [h.random_input(h.DT_HALF, 4099, 9400 + 500 * t + q) for q in range(P)]
        ts = [torch.from_numpy(x).cuda() for x in xs[r]] + [torch.from_numpy(hs16[r]).cuda()]
        with h.config(lib, fusion_pipeline_bytes=64 << 10):
            handles = allreduce_async_batch(ts, names, comm, compression=Compression.bf16_feedback)
            hp = allreduce_async(torch.from_numpy(plain[r]).cuda(), 'fbmp_plain', comm, compression=Compression.bf16)
            got = [hd.wait(timeout=120) for hd in handles] + [hp.wait(timeout=120)]
        stepped = [[f.step(wire, xs[q][i], resid[q][i]) for i in range(len(fb_elems))] for q in range(P)]
        resid = [[stepped[q][i][1] for i in range(len(fb_elems))] for q in range(P)]
        for i, n in enumerate(fb_elems):
            want = f.reduce_ref(ora, wire, [stepped[q][i][0] for q in range(P)], message, w.OP_SUM, P)
            a.assert_same(h.DT_FLOAT, got[i].cpu().numpy(), want, f'round {t}: feedback tensor {i} ({n} elements)')
        a.assert_same(h.DT_HALF, got[2].cpu().numpy(), ora.fold_ref_order(h.DT_HALF, hs16), f'round {t}: the fp16 tensor')
        a.assert_same(h.DT_FLOAT, got[3].cpu().numpy(), w.expected(ora, wire, plain, message, w.OP_SUM, P),
                      f'round {t}: the plain-wire tensor')


def check_feedback_dp_wrapper(ctx):
    """Three step()s of the DP wrapper on a 3-layer fp32 MLP with Compression.bf16_feedback and
    fused_mean=True: after every step every parameter's gradient is the model's value computed from
    the ranks' own gradients (exchanged over the test's gloo group) and the residuals the model
    carried from the steps before. The wrapper's keys are stable per parameter. No div_ runs."""
    import _avg_helpers as a
    import _feedback_helpers as f
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
                                                         compression=Compression.bf16_feedback, fused_mean=True)
    params = list(model.parameters())
    message = 2 * sum(p.numel() for p in params)  # one fp32-over-bf16 plan, keys in parameter order
    resid = [[np.zeros(p.numel(), np.float32) for p in params] for _ in range(P)]
    g = torch.Generator().manual_seed(55 + r)  # its own shard of the batches
    for t in range(ROUNDS):
        x, y = torch.randn(8, 16, generator=g).cuda(), torch.randn(8, 4, generator=g).cuda()
        opt.zero_grad()
        torch.nn.functional.mse_loss(model(x), y).backward()
        theirs = []  # theirs[i][q]: rank q's gradient of parameter i
        for p in params:
            mine = p.grad.detach().cpu().contiguous()
            parts = [torch.empty_like(mine) for _ in range(P)]
            dist.all_gather(parts, mine)
            theirs.append([part.numpy().reshape(-1) for part in parts])
        with _count_div(torch) as divs:
            opt.step()  # (plain SGD leaves p.grad, the reduced gradient, as it is)
        seen = [p.grad.detach().cpu().numpy().reshape(-1).copy() for p in params]
        assert not divs, divs
        stepped = [[f.step(h.DT_BFLOAT16, theirs[i][q], resid[q][i]) for i in range(len(params))] for q in range(P)]
        resid = [[stepped[q][i][1] for i in range(len(params))] for q in range(P)]
        for i in range(len(params)):
            want = f.reduce_ref(ora, h.DT_BFLOAT16, [stepped[q][i][0] for q in range(P)], message, w.OP_AVG, P)
            a.assert_same(h.DT_FLOAT, seen[i], want, f'step {t}: parameter {i}')


FEEDBACK_CHECKS = {fn.__name__: fn for fn in (check_feedback_keyed_batch, check_feedback_dp_wrapper)}


def worker(rank, world, port, q, only):
    _mp_gpu_worker.FAULT_CHECKS.update(FEEDBACK_CHECKS)
    _mp_gpu_worker.worker(rank, world, port, q, only=only, transport='rccl')
