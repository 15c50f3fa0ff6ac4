"""Worker of tests/test_stochastic_multiproc_gpu.py: stochastic rounding of the bf16 wire
(DDL_ALLREDUCE_WIRE_STOCHASTIC) on the whole engine over real multi-rank RCCL on one GPU. The process
setup is tests/_mp_gpu_worker.worker, unchanged; this module only adds its checks to that worker's
table inside the child. Every rank runs the NumPy mirror (_stochastic_helpers) for ALL ranks' inputs —
each rank's wire values from that rank's own stream key — and compares its own results with the oracle's
sum of the wire values, widened and divided on the CPU. Test infrastructure only."""
import numpy as np

import _mp_gpu_worker

STEPS = 2
SEED = 0x5eed0000c0ffee


def check_stochastic_keyed_batch(ctx):
    """Two steps of one batch under the same names: fp32 device tensors of 5, 513 and 70_001 elements with
    Compression.bf16_stochastic and a native fp16 tensor among them (submitted uncompressed). The batch is
    one round and its compressed requests one plan of more than 2048 wire bytes; the 70_001-element tensor
    is cut across 64 KiB sub-plans. Step t is every key's sequence number t."""
    import _avg_helpers as a
    import _feedback_helpers as f
    import _helpers as h
    import _stochastic_helpers as sh
    import _wire_helpers as w
    torch, lib, comm, P, r, ora = ctx['torch'], ctx['lib'], ctx['comm'], ctx['P'], ctx['rank'], ctx['oracle']
    from ddl.torch import Compression
    from ddl.torch.compression import set_stochastic_seed
    from ddl.torch.tensor_communicate import allreduce_async_batch
    elems, names = [5, 513, 70_001], ['srmp_a', 'srmp_b', 'srmp_c']
    message = 2 * sum(elems)
    set_stochastic_seed(SEED)
    for t in range(STEPS):
        xs = [[w.wire_input(n, 9600 + 500 * t + 31 * q + i) for i, n in enumerate(elems)] for q in range(P)]
        hs16 = [h.random_input(h.DT_HALF, 4099, 9700 + 500 * t + q) for q in range(P)]
        ts = [torch.from_numpy(x).cuda() for x in xs[r]]
        ts.insert(1, torch.from_numpy(hs16[r]).cuda())
        with h.config(lib, fusion_pipeline_bytes=64 << 10):
            handles = allreduce_async_batch(ts, names[:1] + ['srmp_half'] + names[1:], comm,
                                            compression=Compression.bf16_stochastic)
            got = [hd.wait(timeout=120) for hd in handles]
        half = got.pop(1)
        a.assert_same(h.DT_HALF, half.cpu().numpy(), ora.fold_ref_order(h.DT_HALF, hs16), f'step {t}: the fp16 tensor')
        for i, n in enumerate(elems):
            ws = [sh.sr(xs[q][i], sh.stream(SEED, q, names[i], t)) for q in range(P)]
            want = f.reduce_ref(ora, h.DT_BFLOAT16, ws, message, w.OP_SUM, P)
            a.assert_same(h.DT_FLOAT, got[i].cpu().numpy(), want, f'step {t}: tensor {i} ({n} elements)')
            if n > 500:  # the ranks round independently: their wire values differ where their inputs agree
                same = sh.sr(xs[0][i], sh.stream(SEED, 0, names[i], t)) == sh.sr(xs[0][i], sh.stream(SEED, 1, names[i], t))
                assert not same.all()


def check_stochastic_dp_wrapper(ctx):
    """One step() of the DP wrapper on a 3-layer fp32 MLP with Compression.bf16_stochastic and
    fused_mean=True: every parameter's gradient is the mirror's value computed from the ranks' own gradients
    (exchanged over the test's gloo group), each rounded with that rank's stream key of the wrapper's name for
    the parameter at sequence number 0. No div_ runs."""
    import _avg_helpers as a
    import _feedback_helpers as f
    import _helpers as h
    import _stochastic_helpers as sh
    import _wire_helpers as w
    from _mp_avg_worker import _count_div
    torch, comm, P, r, ora, dist = ctx['torch'], ctx['comm'], ctx['P'], ctx['rank'], ctx['oracle'], ctx['dist']
    from ddl.torch import Compression
    from ddl.torch.compression import set_stochastic_seed
    from ddl.torch.parallelism.data import data_parallelism_distributed_optimizer_wrapper
    set_stochastic_seed(SEED + 1)
    torch.manual_seed(4321)  # the same weights on every rank
    model = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.Tanh(), torch.nn.Linear(32, 32), torch.nn.Tanh(),
                                torch.nn.Linear(32, 4)).cuda()
    opt = data_parallelism_distributed_optimizer_wrapper(torch.optim.SGD(model.parameters(), lr=0.1), comm,
                                                         compression=Compression.bf16_stochastic, fused_mean=True)
    params = list(model.parameters())
    message = 2 * sum(p.numel() for p in params)  # one fp32-over-bf16 plan, keys in parameter order
    g = torch.Generator().manual_seed(77 + r)  # its own shard of the batch
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
    for i in range(len(params)):
        ws = [sh.sr(theirs[i][q], sh.stream(SEED + 1, q, opt._key(0, i), 0)) for q in range(P)]
        want = f.reduce_ref(ora, h.DT_BFLOAT16, ws, message, w.OP_AVG, P)
        a.assert_same(h.DT_FLOAT, seen[i], want, f'parameter {i}')


STOCHASTIC_CHECKS = {fn.__name__: fn for fn in (check_stochastic_keyed_batch, check_stochastic_dp_wrapper)}


def worker(rank, world, port, q, only):
    _mp_gpu_worker.FAULT_CHECKS.update(STOCHASTIC_CHECKS)
    _mp_gpu_worker.worker(rank, world, port, q, only=only, transport='rccl')
