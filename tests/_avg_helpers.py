"""Expected values of the AVG op (DDL_ALLREDUCE_OP_AVG): the oracle's sum divided on the CPU.

The quotient is numpy's for fp32 / fp64 (`x / np.float32(P)`, `x / np.float64(P)`: the correctly
rounded IEEE quotient), numpy's through float32 for fp16, and torch CPU's for bf16 (stored as raw
uint16, as the other helpers keep it). Never the engine's own output.
"""
import numpy as np
import torch

from _helpers import DT_BFLOAT16, DT_DOUBLE, DT_FLOAT, DT_HALF, NP

FLOAT_DTYPES = [DT_FLOAT, DT_DOUBLE, DT_HALF, DT_BFLOAT16]
OP_SUM, OP_AVG = 0, 1


def quotient(dt, x, P):
    """x / P elementwise as the AVG contract defines it, in x's storage type."""
    x = np.ascontiguousarray(x)
    with np.errstate(all='ignore'):
        if dt == DT_FLOAT:
            return (x / np.float32(P)).astype(np.float32)
        if dt == DT_DOUBLE:
            return (x / np.float64(P)).astype(np.float64)
        if dt == DT_HALF:
            return (x.astype(np.float32) / np.float32(P)).astype(np.float16)
    assert dt == DT_BFLOAT16 and x.dtype == np.uint16
    t = torch.from_numpy(x.view(np.int16).copy()).view(torch.bfloat16)
    return t.div(P).view(torch.int16).numpy().view(np.uint16)


def is_nan(dt, a):
    if dt == DT_BFLOAT16:
        return (a & 0x7fff) > 0x7f80
    return np.isnan(a)


def assert_same(dt, got, want, what=''):
    """Bit-equal wherever `want` is not a NaN; a NaN stays a NaN (its payload is not pinned)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    nan = is_nan(dt, want)
    assert np.array_equal(is_nan(dt, got), nan), f'{what}: NaN positions differ'
    bits = {2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    g, w = got.view(bits)[~nan], want.view(bits)[~nan]
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f'{what}: {bad.size} of {g.size} differ, first at {bad[0]}: {g[bad[0]]:#x} != {w[bad[0]]:#x}'


def to_dev(a, gpu):
    """numpy array (uint16 for bf16) -> device tensor of the same bytes."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to(gpu)


def to_host(t, dt):
    return t.cpu().numpy().view(NP[dt])
