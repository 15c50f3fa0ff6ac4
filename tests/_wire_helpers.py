"""Expected values of the wire compression (ddl_allreduce_wire), computed on the CPU only.

w_q = rank q's fp32 input rounded to the wire type with round-to-nearest-even: numpy's
`astype(np.float16)` for fp16, torch CPU's `.to(torch.bfloat16)` for bf16 (kept as raw uint16, as
the other helpers keep bf16). S = the oracle's sum of the w_q in MPICH's order for the plan's
unpadded WIRE bytes (Oracle.fold_ref_order in the wire dtype). The result is widen(S), which is
exact, divided by np.float32(P) with AVG. Never the engine's own output.
"""
import numpy as np
import torch

from _helpers import DT_BFLOAT16, DT_FLOAT, DT_HALF, random_input

WIRE_FP16, WIRE_BF16 = 0x100, 0x200            # enum ddl_allreduce_wire
WIRE_DT = {WIRE_FP16: DT_HALF, WIRE_BF16: DT_BFLOAT16}
WIRE_NAME = {DT_HALF: 'fp16', DT_BFLOAT16: 'bf16'}
WIRES = [DT_HALF, DT_BFLOAT16]
OP_SUM, OP_AVG = 0, 1

# ties, overflow, underflow, subnormals, signed zero, NaN and inf of both wire types: they tell
# round-to-nearest-even from truncation and from flush-to-zero
SPECIALS = np.array([2049, 2051, 65519, 65520, 1e5, 1e-8, 2.98e-8, 3.0e-8, -0.0, np.nan, -np.inf,
                     1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 3.4e38], dtype=np.float32)


def narrow(wire_dt, x):
    """fp32 array -> the wire type, round to nearest even (fp16 array, or bf16 bits as uint16)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if wire_dt == DT_HALF:
        with np.errstate(all='ignore'):
            return x.astype(np.float16)
    assert wire_dt == DT_BFLOAT16
    return torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def widen(wire_dt, w):
    """The wire values as fp32 (exact)."""
    w = np.ascontiguousarray(w)
    if wire_dt == DT_HALF:
        return w.astype(np.float32)
    assert wire_dt == DT_BFLOAT16 and w.dtype == np.uint16
    return (w.astype(np.uint32) << 16).view(np.float32)


def wire_input(n, seed):
    """A seeded fp32 segment with the special values spliced into its head."""
    x = random_input(DT_FLOAT, n, seed).copy()
    k = min(n, SPECIALS.size)
    x[:k] = SPECIALS[:k]
    return x


def expected(oracle, wire_dt, xs, plan_wire_bytes, op, P):
    """The contract's result for one segment: xs = the ranks' fp32 inputs in rank order."""
    total = oracle.fold_ref_order(wire_dt, [narrow(wire_dt, x) for x in xs], plan_wire_bytes)
    out = widen(wire_dt, total)
    if op == OP_AVG:
        with np.errstate(all='ignore'):
            out = (out / np.float32(P)).astype(np.float32)
    return out


def test_cpu_reference_values():
    """The values the issue pins for numpy's and torch's casts (run as part of the CPU suite by
    tests/test_wire_mirror_cpu.py)."""
    h = narrow(DT_HALF, SPECIALS[:10])
    assert h[:2].tolist() == [2048.0, 2052.0] and h[2] == np.float16(65504) and np.isinf(h[3]) and np.isinf(h[4])
    assert h[5] == 0 and h[6] == 0 and h[7] == np.float16(5.96e-8) and np.signbit(h[8]) and h[8] == 0 and np.isnan(h[9])
    b = widen(DT_BFLOAT16, narrow(DT_BFLOAT16, SPECIALS[11:]))
    assert b[0] == 1.0 and b[1] == 1.015625 and np.isinf(b[2])
