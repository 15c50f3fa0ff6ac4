"""Worker of tests/test_stack_multiproc_gpu.py: the keyed allreduce's options together — error feedback
with prescale / postscale, AVG and the sum of squares, a feedback request that spans fusion plans, and
the data-parallel wrapper with feedback next to gradient_predivide_factor, loss_scale, track_grad_norm
and a skipped step — on the whole engine in several processes on one GPU. The process setup is
tests/_mp_gpu_worker.worker, unchanged; this module only adds its checks to that worker's table inside
the child. Every rank runs the composed CPU model (tests/_stack_helpers.py) for ALL ranks' inputs, round
after round, and also compares its bits with rank 0's. Test infrastructure only."""
import math
import struct

import numpy as np

import _mp_gpu_worker
import _stack_helpers as sh
from _mp_sumsq_worker import _same_as_rank0


def submit_batch(comm, tag, xs, order=None):
    """sh.BATCH under the keys `tag`_...: the feedback requests as one batch, the plain-wire and the
    uncompressed request next to it; `order` permutes the requests (the feedback batch goes where its
    first request stands). Returns (outputs as numpy [request], the spanning request's sum of squares)."""
    import torch
    from ddl.torch import cpp_backend as cb
    from ddl.torch.compression import Compression
    from ddl.torch.tensor_communicate import allreduce_async, allreduce_async_batch
    order = list(range(len(sh.BATCH))) if order is None else list(order)
    ts = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]
    keys = [f'{tag}_{spec[0]}' for spec in sh.BATCH]
    fb = [i for i in order if sh.BATCH[i][2]]
    assert all(sh.BATCH[j][3:5] == (sh.DT_BFLOAT16, sh.OP_AVG) for j in fb)
    handles = {}
    for i in order:
        _, _, feedback, wire, op, a, b, want = sh.BATCH[i]
        if i in handles:
            continue
        if feedback:
            hs = allreduce_async_batch([ts[j] for j in fb], [keys[j] for j in fb], comm, op=cb.OP_AVG,
                                       compression=Compression.bf16_feedback, prescale=[float(sh.BATCH[j][5]) for j in fb],
                                       postscale=[float(sh.BATCH[j][6]) for j in fb], sumsq=[sh.BATCH[j][7] for j in fb])
            handles.update(zip(fb, hs))
        else:
            handles[i] = allreduce_async(ts[i], keys[i], comm, op=op, compression=Compression.bf16 if wire else Compression.none,
                                         prescale=float(a), postscale=float(b), sumsq=want)
    outs = [handles[i].wait(timeout=120).cpu().numpy() for i in range(len(sh.BATCH))]
    for i, spec in enumerate(sh.BATCH):
        assert (handles[i].sumsq is not None) == spec[7]
    return outs, handles[sh.SPANNING].sumsq


def check_round(outs, sq, want_outs, want_sqs, what):
    for i, (got, want) in enumerate(zip(outs, want_outs)):
        assert sh.same_bits(got, want), f'{what}: request {sh.BATCH[i][0]} ({got.size} elements)'
    assert sh.same_double(sq, want_sqs[sh.SPANNING]), (what, sq, want_sqs[sh.SPANNING])


def _raw(arrays):
    """Bytes to compare with rank 0: the values with the NaNs zeroed, and where the NaNs are."""
    return b''.join(np.where(np.isnan(a), np.float32(0), a).tobytes() + np.isnan(a).tobytes() for a in arrays)


def check_stack_keyed(ctx):
    """sh.BATCH at real P under 64 KiB plans, three rounds under the same keys, every rank submitting in
    its own permutation: the 70_001-element feedback request spans three plans, so its residual is
    handed on at elem_begin; the handler's residuals show through the outputs of rounds 2 and 3."""
    import _helpers as h
    lib, comm, P, r, ora = ctx['lib'], ctx['comm'], ctx['P'], ctx['rank'], ctx['oracle']
    order = [int(i) for i in np.random.default_rng(5 + r).permutation(len(sh.BATCH))]
    resid, raw = sh.batch_zero_residuals(P), b''
    with h.config(lib, fusion_threshold_bytes=sh.LIMIT, fusion_pipeline_bytes=0):
        for t in range(sh.ROUNDS):
            xs = sh.batch_inputs(P, t)
            want_outs, resid, want_sqs = sh.batch_round(ora, P, xs, resid)
            outs, sq = submit_batch(comm, 'stkmp', xs[r], order)
            check_round(outs, sq, want_outs, want_sqs, f'round {t + 1}')
            raw += _raw(outs) + (b'nan' if math.isnan(sq) else struct.pack('<d', sq))
        assert math.isfinite(sq)
    _same_as_rank0(ctx, raw, 'stacked keyed batch')


def check_stack_wrapper(ctx):
    """The data-parallel wrapper on a 3-layer MLP with Compression.bf16_feedback, fused_mean,
    gradient_predivide_factor = 2, track_grad_norm and DynamicLossScaler(init_scale=1024,
    growth_interval=2), four steps on the step() path and four with the overlap_backward hooks. The ranks'
    raw gradients are exchanged over the test's gloo group before each step; after it every p.grad equals
    the model's value bit for bit — its residuals carried in prescaled units (g / 2 of the SCALED loss)
    — and grad_norm equals sqrt(fsum(mirror(...))) as a double. The second step overflows on the last
    rank only: every rank skips it, the parameters stay, the scale is halved, and the third step's
    gradients are the model's, whose residuals advanced on the clean ranks, were cleared on the last one,
    and meet the new scale's postscale. No div_ runs.

    The hooks submit every gradient on its own, so a plan may be one small gradient; at P <= 3 MPICH's
    order is the same on both sides of its 2048-byte switch, so the model's one message size holds."""
    import _helpers as h
    from _mp_avg_worker import _count_div
    torch, lib, comm, P, r, ora, dist = (ctx[k] for k in ('torch', 'lib', 'comm', 'P', 'rank', 'oracle', 'dist'))
    from ddl.torch import Compression
    from ddl.torch.parallelism.data import DynamicLossScaler
    from ddl.torch.parallelism.data.distributed_optimizer import data_parallelism_distributed_optimizer_wrapper as wrap
    assert P <= 3
    raw = b''
    with h.config(lib, fusion_pipeline_bytes=0):
        for overlap in (False, True):
            model = sh.mlp(torch, 'cuda')
            opt = wrap(torch.optim.SGD(model.parameters(), lr=0.1), comm, overlap_backward=overlap, bucket_bytes=None,
                       compression=Compression.bf16_feedback, fused_mean=True, gradient_predivide_factor=sh.PREDIVIDE,
                       track_grad_norm=True)
            scaler = DynamicLossScaler(opt, init_scale=sh.INIT_SCALE, growth_interval=2)
            params = list(model.parameters())
            resid = [[np.zeros(p.numel(), np.float32) for p in params] for _ in range(P)]
            gen, scales = sh.shard(torch, r), []
            for t in range(sh.STEPS):
                what = f'overlap {overlap} step {t + 1}'
                S = scaler.loss_scale
                scales.append(S)
                before = [p.detach().clone() for p in params]
                opt.zero_grad()
                loss = scaler.scale(sh.loss_of(torch, model, gen, 'cuda', t == sh.INF_STEP and r == P - 1))
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
                seen = [p.grad.detach().cpu().numpy().reshape(-1).copy() for p in params]
                old = resid
                want, resid, norm = sh.wrapper_round(ora, P, theirs, resid, S)
                for i in range(len(params)):
                    assert sh.same_bits(seen[i], want[i]), f'{what}: parameter {i}'
                assert sh.same_double(opt.grad_norm, norm), (what, opt.grad_norm, norm)
                if t == sh.INF_STEP:
                    assert taken is False and opt.found_nonfinite and not math.isfinite(norm), what
                    assert scaler.loss_scale == S / 2 == opt.loss_scale
                    assert all(torch.equal(p.detach(), b) for p, b in zip(params, before)), what
                    assert not any(np.isfinite(theirs[i][P - 1]).any() for i in range(len(params)))
                    assert all(np.isfinite(theirs[i][q]).all() for i in range(len(params)) for q in range(P - 1))
                else:
                    assert taken is True and not opt.found_nonfinite and math.isfinite(norm) and norm > 0, what
                    assert not all(torch.equal(p.detach(), b) for p, b in zip(params, before)), what
                if t == sh.INF_STEP + 1:
                    # these gradients tell the model from an engine that dropped the residuals on the skipped
                    # step, or kept the last rank's where its values were not finite (a check of the inputs)
                    assert any(old[q][i].any() for q in range(P - 1) for i in range(len(params)))
                    assert not any(old[P - 1][i].any() for i in range(len(params)))
                    zero = [[np.zeros_like(x) for x in row] for row in old]
                    dropped, _, _ = sh.wrapper_round(ora, P, theirs, zero, S)
                    assert any(not sh.same_bits(a, b) for a, b in zip(dropped, want)), what
                raw += _raw(seen) + (b'nan' if math.isnan(norm) else struct.pack('<d', opt.grad_norm))
            assert scales == [1024.0, 1024.0, 512.0, 512.0] and scaler.loss_scale == 1024.0
            for hook in getattr(opt, '_hooks', []):
                hook.remove()
    _same_as_rank0(ctx, raw, 'stacked wrapper')


STACK_CHECKS = {f.__name__: f for f in (check_stack_keyed, check_stack_wrapper)}


def worker(rank, world, port, q, only, transport):
    _mp_gpu_worker.FAULT_CHECKS.update(STACK_CHECKS)
    _mp_gpu_worker.worker(rank, world, port, q, only=only, transport=transport)
