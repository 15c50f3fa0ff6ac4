"""Worker of tests/test_e4m3_multiproc_gpu.py: the e4m3 wire (DDL_ALLREDUCE_WIRE_E4M3) on the whole engine in
several processes on one GPU. The process setup is tests/_mp_gpu_worker.worker, unchanged; this module only adds
its checks to that worker's table inside the child. Every rank runs the CPU model (tests/_e4m3_helpers.py) for ALL
ranks' inputs and also compares its bits with rank 0's. Test infrastructure only."""
import math
import struct

import numpy as np

import _e4m3_helpers as q8
import _mp_gpu_worker
from _mp_stack_worker import _raw
from _mp_sumsq_worker import _same_as_rank0

THIRD = float(np.float32(1) / np.float32(3))


def check_e4m3_keyed_mix(ctx):
    """One keyed round of three batches submitted back to back, every rank in its own order: fp8 requests (SUM and
    AVG by batch, factors and the statistic per request, a native fp16 tensor among them), bf16-wire requests and
    plain fp32 requests. 64 KiB sub-plans cut the 70_001-element fp8 request."""
    import _avg_helpers as a
    import _feedback_helpers as f
    import _helpers as h
    import _wire_helpers as w
    from _sumsq_helpers import mirror
    torch, lib, comm, P, r, ora = ctx['torch'], ctx['lib'], ctx['comm'], ctx['P'], ctx['rank'], ctx['oracle']
    from ddl.torch import Compression, cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async_batch
    elems = [5, 253, 70_001, 1009]
    pre, post, wish = [1.0, THIRD, 0.5, 1.0], [1.0, 1.0, THIRD, 3.0], [True, False, True, True]
    xs = [[q8.rank_input(n, 300 + i, q, specials=i < 2) for i, n in enumerate(elems)] for q in range(P)]
    hs16 = [h.random_input(h.DT_HALF, 4099, 9800 + q) for q in range(P)]
    bf = [[w.wire_input(n, 9900 + 31 * q + i) for i, n in enumerate((300, 4099))] for q in range(P)]
    plain = [[h.random_input(h.DT_FLOAT, n, 9950 + 31 * q + i) for i, n in enumerate((7, 5000))] for q in range(P)]

    def dev(v):
        return torch.from_numpy(v).cuda()
    with h.config(lib, fusion_pipeline_bytes=64 << 10):
        def fp8():
            ts = [dev(x) for x in xs[r]] + [dev(hs16[r])]
            return allreduce_async_batch(ts, [f'q8mp_{i}' for i in range(len(elems))] + ['q8mp_half'], comm, op=cb.OP_AVG,
                                         compression=Compression.fp8, prescale=pre + [1.0], postscale=post + [1.0],
                                         sumsq=wish + [False])

        def bf16():
            return allreduce_async_batch([dev(x) for x in bf[r]], ['q8mp_bf0', 'q8mp_bf1'], comm, compression=Compression.bf16)

        def fp32():
            return allreduce_async_batch([dev(x) for x in plain[r]], ['q8mp_p0', 'q8mp_p1'], comm)
        order = [fp8, bf16, fp32]
        handles = {fn.__name__: fn() for fn in (order if r % 2 == 0 else order[::-1])}
        got = {k: [hd.wait(timeout=120) for hd in v] for k, v in handles.items()}
    raw = b''
    cuts = q8.subplan_cuts(elems, 64 << 10)  # the requests are one plan, in key order
    assert cuts[2] and not cuts[3]
    for i, n in enumerate(elems):
        want = q8.allreduce([xs[q][i] for q in range(P)], q8.OP_AVG, pre[i], post[i])
        out = got['fp8'][i].cpu().numpy()
        a.assert_same(h.DT_FLOAT, out, want, f'fp8 request {i} ({n} elements)')
        sq = handles['fp8'][i].sumsq
        assert (sq is not None) == wish[i]
        if wish[i]:
            m = mirror(out, False, cuts[i])
            assert (math.isnan(m) and math.isnan(sq)) or struct.pack('<d', sq) == struct.pack('<d', m), (i, sq, m, cuts[i])
            assert math.isnan(m) == (i == 0)
        raw += _raw([out])
    a.assert_same(h.DT_HALF, got['fp8'][-1].cpu().numpy(), a.quotient(h.DT_HALF, ora.fold_ref_order(h.DT_HALF, hs16), P),
                  'the fp16 tensor of the fp8 batch')
    message = 2 * (300 + 4099)
    for i in range(2):
        ws = [w.narrow(h.DT_BFLOAT16, bf[q][i]) for q in range(P)]
        want = f.reduce_ref(ora, h.DT_BFLOAT16, ws, message, w.OP_SUM, P)
        a.assert_same(h.DT_FLOAT, got['bf16'][i].cpu().numpy(), want, f'bf16-wire request {i}')
    for i in range(2):
        want = ora.fold_ref_order(h.DT_FLOAT, [plain[q][i] for q in range(P)], 4 * (7 + 5000))
        a.assert_same(h.DT_FLOAT, got['fp32'][i].cpu().numpy(), want, f'plain request {i}')
    _same_as_rank0(ctx, raw, 'e4m3 keyed mix')


def check_e4m3_wrapper(ctx):
    """The data-parallel wrapper on a 3-layer fp32 MLP with Compression.fp8, fused_mean, gradient_predivide_factor
    2, track_grad_norm and DynamicLossScaler over three steps, on the step() path and on the overlap_backward hooks.
    The ranks' raw gradients are exchanged over the test's gloo group before each step; after it every p.grad is the
    model's value bit for bit and grad_norm is sqrt(fsum(uncompressed sums of squares)) as a double. No div_ runs."""
    import _helpers as h
    import _stack_helpers as sh
    from _mp_avg_worker import _count_div
    from _sumsq_helpers import mirror
    torch, lib, comm, P, r, dist = (ctx[k] for k in ('torch', 'lib', 'comm', 'P', 'rank', 'dist'))
    from ddl.torch import Compression
    from ddl.torch.parallelism.data import DynamicLossScaler
    from ddl.torch.parallelism.data.distributed_optimizer import data_parallelism_distributed_optimizer_wrapper as wrap
    raw, F = b'', 2.0
    with h.config(lib, fusion_pipeline_bytes=0):
        for overlap in (False, True):
            model = sh.mlp(torch, 'cuda')
            opt = wrap(torch.optim.SGD(model.parameters(), lr=0.1), comm, overlap_backward=overlap, bucket_bytes=None,
                       compression=Compression.fp8, fused_mean=True, gradient_predivide_factor=F, track_grad_norm=True)
            scaler = DynamicLossScaler(opt, init_scale=1024.0, growth_interval=2)
            params = list(model.parameters())
            gen = sh.shard(torch, r)
            for t in range(3):
                what = f'overlap {overlap} step {t + 1}'
                S = scaler.loss_scale
                opt.zero_grad()
                loss = scaler.scale(sh.loss_of(torch, model, gen, 'cuda', False))
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
                with _count_div(torch) as divs:
                    if overlap:
                        loss.backward()
                    taken = scaler.step()
                assert not divs, divs
                assert taken is True and not opt.found_nonfinite, what
                seen = [p.grad.detach().cpu().numpy().reshape(-1).copy() for p in params]
                a, b = float(np.float32(1.0 / F)), float(np.float32(F * (1.0 / S)))
                sqs = []
                for i in range(len(params)):
                    want = q8.allreduce(theirs[i], q8.OP_AVG, a, b)
                    assert seen[i].tobytes() == want.tobytes(), f'{what}: parameter {i}'
                    sqs.append(mirror(want, False))
                norm = math.sqrt(math.fsum(sqs))
                assert struct.pack('<d', opt.grad_norm) == struct.pack('<d', norm), (what, opt.grad_norm, norm)
                raw += _raw(seen) + struct.pack('<d', opt.grad_norm)
            assert scaler.loss_scale == 2048.0  # two clean steps doubled it, the third ran under the new scale
            for hook in getattr(opt, '_hooks', []):
                hook.remove()
    _same_as_rank0(ctx, raw, 'e4m3 wrapper')


def check_e4m3_tuned(ctx):
    """The autotuner on (the production default; collective timing, max over ranks through the transport): fp8 requests
    of two size classes, each submitted twice — the first tunes its class with the granule dtype (zeroed granules through
    every candidate), the second runs the chosen schedule again. Every result is the model's bits and rank 0's, every
    rank holds the same table, at P > 2 no candidate is a ring, and the tables sit in classes of the wire's own: the
    summing dtypes' class of the same bytes stays untuned."""
    import ctypes

    import _avg_helpers as a
    import _helpers as h
    torch, lib, comm, P, r, dist = (ctx[k] for k in ('torch', 'lib', 'comm', 'P', 'rank', 'dist'))
    from ddl.torch import Compression, cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async
    raw, picks = b'', []
    with h.config(lib, tune=1, fusion_pipeline_bytes=0):
        for j, n in enumerate((1009, 300_001)):
            xs = [q8.rank_input(n, 500 + j, q) for q in range(P)]
            want = q8.allreduce(xs, q8.OP_AVG, THIRD, 3.0)
            for rep in range(2):
                out = allreduce_async(torch.from_numpy(xs[r]).cuda(), f'q8tune_{j}_{rep}', comm, op=cb.OP_AVG,
                                      compression=Compression.fp8, prescale=THIRD, postscale=3.0).wait(timeout=160)
                a.assert_same(h.DT_FLOAT, out.cpu().numpy(), want, f'tuned fp8 request of {n} elements, run {rep}')
                raw += _raw([out.cpu().numpy()])
            wire_bytes = q8.granules(n) * q8.GRANULE
            chosen, count = ctypes.c_int(-1), ctypes.c_int(0)
            cfgs, tms = (ctypes.c_longlong * 256)(), (ctypes.c_float * 64)()
            cb.check(lib.ddl_testing_keyed_tune_result(comm.id, wire_bytes, 1, ctypes.byref(chosen), ctypes.byref(count), cfgs,
                                                       tms, 64), 'ddl_testing_keyed_tune_result')
            assert 0 <= chosen.value < count.value and count.value >= 2, (chosen.value, count.value)
            algos = [int(cfgs[4 * i]) for i in range(count.value)]
            assert P == 2 or 0 not in algos, algos  # a ring at P > 2 would fold more than once
            picks.append((chosen.value, algos, [round(tms[i], 6) for i in range(count.value)]))
            plain, pc = ctypes.c_int(-1), ctypes.c_int(-1)
            cb.check(lib.ddl_testing_keyed_tune_result(comm.id, wire_bytes, 0, ctypes.byref(plain), ctypes.byref(pc), None, None, 0),
                     'ddl_testing_keyed_tune_result')
            assert pc.value == 0, pc.value
    everyone = [None] * P
    dist.all_gather_object(everyone, picks)
    assert all(e == picks for e in everyone), everyone  # the same choice and the same agreed times
    _same_as_rank0(ctx, raw, 'tuned e4m3 requests')


E4M3_CHECKS = {f.__name__: f for f in (check_e4m3_keyed_mix, check_e4m3_wrapper, check_e4m3_tuned)}


def worker(rank, world, port, q, only, transport):
    _mp_gpu_worker.FAULT_CHECKS.update(E4M3_CHECKS)
    _mp_gpu_worker.worker(rank, world, port, q, only=only, transport=transport)
