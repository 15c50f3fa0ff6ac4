"""The low-rank wire's reference (include/ddl_amd.h "The low-rank wire" in plain NumPy, fp64 by default, the dtype a
parameter so the same code also runs in fp32), the thread-world runner, and the worker of test_lowrank_gpu.py's
processes: _mp_gpu_worker.worker with check_lowrank_batch added inside the child."""
import ctypes

import numpy as np

import _mp_gpu_worker
from _mp_minmax_worker import _same_as_rank0

SUM, AVG, NAN = 0, 1, 0x7fc00000
LENGTHS = (1, 63, 4096, 4099, 70001, 1 << 20)  # two that travel whole, exact tiles, ragged, 219 x 320, two K-splits


def shape(n, r):
    """(R, C, small) of n elements at rank r."""
    m = 1
    while (64 * m) ** 2 < n:
        m += 1
    R = -(-n // (64 * m))
    return R, 64 * m, 2 * r * (R + 64 * m) > n


def qinit(C, r):
    x = ((16 * np.arange(C, dtype=np.uint64)[:, None] + np.arange(r, dtype=np.uint64) + 0x9e3779b9) & 0xffffffff).astype(np.uint32)
    for shift, mul in ((16, 0x85ebca6b), (13, 0xc2b2ae35), (16, 1)):
        x = ((x ^ (x >> np.uint32(shift))).astype(np.uint64) * mul & 0xffffffff).astype(np.uint32)
    return x.view(np.int32).astype(np.float32) * np.float32(2.0 ** -31)


class State:
    """Of one name: every rank's error, and the Q and flags all ranks share."""
    def __init__(self, n, r, P):
        R, C, self.small = shape(n, r)
        self.e, self.q, self.flags = [np.zeros(n, np.float32) for _ in range(P)], np.zeros((C, r)), np.zeros(r, bool)


def step(gs, st, r, op=SUM, pre=1.0, post=1.0, dt=np.float64):
    """One step of one tensor, st updated in place -> (out, a per rank). Products in `dt`, the dots in fp64."""
    P, n = len(gs), gs[0].size
    R, C, small = shape(n, r)
    scaled = [g if pre == 1.0 else g * np.float32(pre) for g in gs]
    with np.errstate(all='ignore'):
        if small:
            out = np.sum(scaled, axis=0, dtype=dt)
            return ((out / dt(P) if op == AVG else out) * dt(post)).astype(dt), scaled
        a = [(s + e).astype(dt) for s, e in zip(scaled, st.e)]  # (the fp32 sum, rounded once, whatever dt is)
        A = [np.concatenate([x, np.zeros(R * C - n, dt)]).reshape(R, C) for x in a]
        p = np.sum([m @ np.where(st.flags, st.q, qinit(C, r)).astype(dt) for m in A], axis=0)
        flags, poison = np.zeros(r, bool), False
        for j in range(r):
            for i in range(j):
                p[:, j] = (p[:, j].astype(np.float64) - (p[:, i].astype(np.float64) @ p[:, j].astype(np.float64)) * p[:, i]).astype(dt)
            s = p[:, j].astype(np.float64) @ p[:, j].astype(np.float64)
            poison |= not np.isfinite(s)
            flags[j] = np.isfinite(s) and s != 0
            p[:, j] = (p[:, j].astype(np.float64) / np.sqrt(s)).astype(dt) if flags[j] else 0
        q = np.sum([m.T @ p for m in A], axis=0) / dt(P)
        if poison or not np.isfinite(q).all():
            return np.full(n, np.nan, dt), a
        d = (p @ q.T).reshape(-1)[:n]
        left = a - d
        st.e = [np.where(np.isfinite(x), x, 0).astype(np.float32) for x in left]
        st.q, st.flags = q.astype(np.float32), flags
        return ((d if op == AVG else d * dt(P)) * dt(post)).astype(dt), a


def signal(n, r, P, seed, noise=2.0 ** -10):
    """gs[q]: rank r per rank, singular values 1 .. 8, one row space for all ranks and steps, plus noise."""
    R, C, small = shape(n, r)
    rng = np.random.default_rng(seed)
    if small:
        return [rng.standard_normal(n).astype(np.float32) for _ in range(P)]
    v = np.linalg.qr(np.random.default_rng(n + r).standard_normal((C, r)))[0] * np.linspace(1, 8, r)
    gs = []
    for _ in range(P):
        m = np.linalg.qr(rng.standard_normal((R, r)))[0] @ v.T * np.sqrt(R * C / r)
        gs.append((m + noise * np.sqrt(np.mean(m * m)) * rng.standard_normal((R, C))).reshape(-1)[:n].astype(np.float32))
    return gs


def rel(x, want):
    """The largest difference relative to the largest wanted magnitude."""
    return float(np.abs(x.astype(np.float64) - want).max() / max(np.abs(want).max(), 1e-300))


def close(got, want, floor, a=None, post=1.0):
    """got is want within 4 times `floor` (rel() of the restatement in fp32). A tensor that travels whole (a given) is
    a plain fp32 sum whose floor may be 0 by luck: any order errs by at most (P + 1) 2^-24 sum |a| per element."""
    if a is None:
        return rel(got, want) <= 4 * floor
    slack = (len(a) + 1) * 2.0 ** -24 * post * np.sum(np.abs(a), axis=0, dtype=np.float64)
    return bool((np.abs(got.astype(np.float64) - want) <= slack).all())


def padded(x, offset=0):
    """x on the device between guard elements of 7.0; offset 1: it starts 4 bytes behind a 16-byte boundary."""
    import torch
    t = torch.full((x.size + 6,), 7.0, device='cuda')[4 + offset:4 + offset + x.size]
    return t.copy_(torch.from_numpy(x.astype(np.float32)))


def device_state(lib, n, P, offset=0):
    """Fresh residuals and Q states of one name for P ranks, sized by ddl_testing_lowrank_shape at the configured r."""
    r, out = lib.ddl_get_config(b'wire_lowrank_rank'), [ctypes.c_size_t() for _ in range(3)]
    assert lib.ddl_testing_lowrank_shape(n, r, *[ctypes.byref(o) for o in out]) == 0, lib.ddl_last_error()
    assert (out[0].value, out[1].value, out[2].value == 0) == shape(n, r) and out[2].value in (0, out[1].value * r + r)
    return ([padded(np.zeros(n, np.float32), offset) for _ in range(P)],
            [padded(np.zeros(max(out[2].value, 1), np.float32)) for _ in range(P)])


def run_thread_lowrank(lib, xs, res, qs, op=SUM, pre=None, post=None, offset=0):
    """ddl_testing_thread_lowrank over xs[r][i]; res and qs (padded()) rewritten in place; returns outs[r][i]."""
    import torch
    P, k = len(xs), len(xs[0])
    ins, outs = [[[padded(x, offset) for x in row] for row in xs] for _ in range(2)]
    ptrs = [(ctypes.c_void_p * (P * k))(*[t.data_ptr() for row in ts for t in row]) for ts in (ins, outs, res, qs)]
    fa = [None if f is None else (ctypes.c_float * (P * k))(*([f] * (P * k))) for f in (pre, post)]
    assert lib.ddl_testing_thread_lowrank(P, k, *ptrs, (ctypes.c_size_t * k)(*[x.size for x in xs[0]]), fa[0], fa[1], op,
                                          torch.cuda.current_stream().cuda_stream) == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    for t in (t for ts in (outs, res, qs) for row in ts for t in row):
        assert t._base[t.storage_offset() - 1] == 7.0 == t._base[t.storage_offset() + t.numel()], 'a guard was overwritten'
    return [[t.cpu().numpy() for t in row] for row in outs]


def check_lowrank_batch(ctx):
    """Two steps of a Compression.powersgd AVG batch beside a SUM batch: close() to the rule, ranks bit-equal."""
    torch, comm, P, r = ctx['torch'], ctx['comm'], ctx['P'], ctx['rank']
    from ddl.torch import Compression, cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async_batch
    sizes, names = (5, 4099, 70001), ['lr0', 'lr1', 'lr2']
    st64, st32 = [[State(n, 4, P) for n in sizes] for _ in range(2)]
    for it in range(2):
        xs = [signal(n, 4, P, 100 * it + i) for i, n in enumerate(sizes)]
        ks = [np.random.default_rng(90 + q).integers(-8, 9, 300).astype(np.float32) for q in range(P)]
        hs = allreduce_async_batch([torch.from_numpy(x[r]).cuda() for x in xs], names, comm, op=cb.OP_AVG,
                                   compression=Compression.powersgd)
        plain = allreduce_async_batch([torch.from_numpy(ks[r]).cuda()], ['sum0'], comm)
        got = [h.wait(timeout=120) for h in hs]
        assert np.array_equal(plain[0].wait(timeout=120).cpu().numpy(), np.sum(ks, axis=0))
        for i in range(3):
            want, a = step(xs[i], st64[i], 4, AVG)
            floor = rel(step(xs[i], st32[i], 4, AVG, dt=np.float32)[0], want)
            assert close(got[i].cpu().numpy(), want, floor, a if st64[i].small else None), (it, i, floor)
        _same_as_rank0(ctx, got, 'lowrank batch')


def worker(rank, world, port, q, only, transport):
    _mp_gpu_worker.FAULT_CHECKS['check_lowrank_batch'] = check_lowrank_batch
    _mp_gpu_worker.worker(rank, world, port, q, only=only, transport=transport)
