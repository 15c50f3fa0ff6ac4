"""The top-k wire's reference (include/ddl_amd.h "The top-k wire" in plain numpy fp32) and the thread-world runner."""
import ctypes

import numpy as np

SUM, AVG = 0, 1
LENGTHS = (1, 5, 2047, 2048, 2049, 70_001)  # both sides of a tile edge, 35 tiles, k = 1 and k = n


def count(n, ppm):
    return min(n, max(1, -(-n * ppm // 10 ** 6)))


def reference(gs, rs, ppm, op=SUM, pre=1.0, post=1.0):
    """One tensor: gs[q], rs[q] per rank -> (out, new residuals). np.float32 operations only, each rounded once."""
    P, n = len(gs), gs[0].size
    out, new = np.zeros(n, np.float32), []
    with np.errstate(all='ignore'):
        for g, r in zip(gs, rs):
            a = (g if pre == 1.0 else g * np.float32(pre)) + r
            key = a.view(np.uint32) & np.uint32(0x7fffffff)
            sel = np.sort(np.lexsort((np.arange(n), -key.astype(np.int64)))[:count(n, ppm)])  # (-key, index), stable
            out[sel] += a[sel]  # in rank order; indices are unique within a rank
            keep = a.copy()
            keep[sel] = 0.0
            new.append(keep)
        if op == AVG:
            out = out / np.float32(P)
        if post != 1.0:
            out = out * np.float32(post)
    return out, new


def run_thread_topk(lib, xs, res, op=SUM, pre=None, post=None, offset_out=False):
    """ddl_testing_thread_topk over xs[r][i] with the residuals res[r][i] (device tensors, rewritten in place);
    returns outs[r][i]. offset_out: every output starts 4 bytes behind a 16-byte boundary."""
    import torch
    P, k = len(xs), len(xs[0])
    ins = [[torch.from_numpy(x).cuda() for x in row] for row in xs]
    bufs = [[torch.full((x.size + 1,), 7.0, device='cuda') for x in row] for row in xs]
    outs = [[b[1:] if offset_out else b[:-1] for b in row] for row in bufs]
    ptrs = [(ctypes.c_void_p * (P * k))(*[t.data_ptr() for row in ts for t in row]) for ts in (ins, outs, res)]
    fa = [None if f is None else (ctypes.c_float * (P * k))(*([f] * (P * k))) for f in (pre, post)]
    assert lib.ddl_testing_thread_topk(P, k, ptrs[0], ptrs[1], ptrs[2], (ctypes.c_size_t * k)(*[x.size for x in xs[0]]),
                                       fa[0], fa[1], op, torch.cuda.current_stream().cuda_stream) == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    return [[t.cpu().numpy() for t in row] for row in outs]
