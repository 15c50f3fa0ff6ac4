"""The sign wire's reference (include/ddl_amd.h "The sign wire" in plain numpy fp32), the thread-world runner, and the
worker of test_sign_gpu.py's processes: _mp_gpu_worker.worker with check_sign_batch added inside the child."""
import ctypes

import numpy as np

import _mp_gpu_worker
from _mp_minmax_worker import _same_as_rank0

SUM, AVG, BLOCK, NAN = 0, 1, 2048, 0x7fc00000
LENGTHS = (1, 63, 2047, 2048, 2049, 4 * 2048 + 5)  # a lone element, a short row, both sides of a block edge, 5 blocks


def reference(gs, rs, op=SUM, pre=1.0, post=1.0):
    """One tensor: gs[q], rs[q] per rank -> (out, new residuals). np.float32 operations only, each rounded once."""
    P, n = len(gs), gs[0].size
    nb = -(-n // BLOCK)
    acc, bad, new = np.zeros(nb * BLOCK, np.float32), np.zeros(nb, bool), []
    c = np.minimum(n - BLOCK * np.arange(nb), BLOCK).astype(np.float32)
    with np.errstate(all='ignore'):
        for g, r in zip(gs, rs):
            a, old = np.zeros(nb * BLOCK, np.float32), np.zeros(nb * BLOCK, np.float32)
            a[:n], old[:n] = (g if pre == 1.0 else g * np.float32(pre)) + r, r
            # element row * 256 + 4 w + j of a block is bit k = 4 row + j of word w
            m = np.abs(a).reshape(nb, 8, 64, 4).transpose(0, 2, 1, 3).reshape(nb, 64, 32)
            t = np.zeros((nb, 64), np.float32)
            for k in range(32):
                t = t + m[:, :, k]
            for d in (32, 16, 8, 4, 2, 1):
                t = t + t[:, np.arange(64) ^ d]
            s = t[:, 0] / c
            fin = np.isfinite(s)
            bad |= ~fin
            sent = np.copysign(np.repeat(np.where(fin, s, np.float32(0)), BLOCK), a)  # the IEEE sign bit of a
            acc = acc + sent  # in rank order, from +0.0
            new.append(np.where(np.repeat(fin, BLOCK), a - sent, old)[:n])
        out = acc / np.float32(P) if op == AVG else acc.copy()
        if post != 1.0:
            out = out * np.float32(post)
    out.view(np.uint32)[np.repeat(bad, BLOCK)] = NAN
    return out[:n], new


def padded(x, offset=0):
    """x on the device between two guard elements of 7.0; offset 1: it starts 4 bytes behind a 16-byte boundary."""
    import torch
    t = torch.full((x.size + 6,), 7.0, device='cuda')[4 + offset:4 + offset + x.size]
    return t.copy_(torch.from_numpy(x))


def run_thread_sign(lib, xs, res, op=SUM, pre=None, post=None, offset=0):
    """ddl_testing_thread_sign over xs[r][i] with the residuals res[r][i] (padded() tensors, rewritten in place);
    returns outs[r][i]. Nothing may be written outside an output or a residual."""
    import torch
    P, k = len(xs), len(xs[0])
    ins, outs = [[[padded(x, offset) for x in row] for row in xs] for _ in range(2)]
    ptrs = [(ctypes.c_void_p * (P * k))(*[t.data_ptr() for row in ts for t in row]) for ts in (ins, outs, res)]
    fa = [None if f is None else (ctypes.c_float * (P * k))(*([f] * (P * k))) for f in (pre, post)]
    assert lib.ddl_testing_thread_sign(P, k, ptrs[0], ptrs[1], ptrs[2], (ctypes.c_size_t * k)(*[x.size for x in xs[0]]),
                                       fa[0], fa[1], op, torch.cuda.current_stream().cuda_stream) == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    for t in (t for ts in (outs, res) for row in ts for t in row):
        assert t._base[t.storage_offset() - 1] == 7.0 == t._base[t.storage_offset() + t.numel()], 'a guard was overwritten'
    return [[t.cpu().numpy() for t in row] for row in outs]


def check_sign_batch(ctx):
    """Two steps of a Compression.onebit AVG batch under stable names beside a SUM batch: the numpy rule bit for bit."""
    torch, comm, P, r = ctx['torch'], ctx['comm'], ctx['P'], ctx['rank']
    from ddl.torch import Compression, cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async_batch
    sizes, names = (5, 4099, 300), ['sign0', 'sign1', 'sign2']
    res = [[np.zeros(n, np.float32) for n in sizes] for _ in range(P)]
    for step in range(2):
        xs = [[np.random.default_rng(100 * step + 10 * q + i).standard_normal(n).astype(np.float32)
               for i, n in enumerate(sizes)] for q in range(P)]
        ks = [np.random.default_rng(90 + q).integers(-8, 9, 300).astype(np.float32) for q in range(P)]
        signs = allreduce_async_batch([torch.from_numpy(x).cuda() for x in xs[r]], names, comm, op=cb.OP_AVG,
                                      compression=Compression.onebit)
        plain = allreduce_async_batch([torch.from_numpy(ks[r]).cuda()], ['sum0'], comm)
        got = [h.wait(timeout=120) for h in signs]
        assert np.array_equal(plain[0].wait(timeout=120).cpu().numpy(), np.sum(ks, axis=0))
        for i in range(3):
            want, new = reference([x[i] for x in xs], [row[i] for row in res], AVG)
            res = [row[:i] + [new[q]] + row[i + 1:] for q, row in enumerate(res)]
            assert got[i].cpu().numpy().tobytes() == want.tobytes(), (step, i)
        _same_as_rank0(ctx, got, 'sign batch')


def worker(rank, world, port, q, only, transport):
    _mp_gpu_worker.FAULT_CHECKS['check_sign_batch'] = check_sign_batch
    _mp_gpu_worker.worker(rank, world, port, q, only=only, transport=transport)
