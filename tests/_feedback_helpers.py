"""CPU model of the wire's error feedback (DDL_ALLREDUCE_WIRE_FEEDBACK), numpy only.

Per element, with r the rank's residual for the key (zero the first time), all arithmetic in fp32
with round-to-nearest-even and subnormals kept:

    v  = g + r
    w  = narrow(v)                          (_wire_helpers.narrow: numpy's fp16 / torch CPU's bf16 cast)
    r' = isfinite(widen(w)) ? v - widen(w) : 0

w goes to the wire, r' replaces r. From there on the request is the compressed request of
_wire_helpers.expected: the oracle's sum of the ranks' w in MPICH's order for the plan's unpadded
wire bytes, widened, divided by np.float32(P) with AVG. Never the engine's own output.
"""
import numpy as np

from _helpers import DT_BFLOAT16, DT_HALF
from _wire_helpers import OP_AVG, SPECIALS, narrow, widen

WIRE_FEEDBACK = 0x1000  # enum ddl_allreduce_wire


def step(wire_dt, g, r):
    """One application of the rule: (w in the wire type, r' as fp32)."""
    g, r = np.ascontiguousarray(g, dtype=np.float32), np.ascontiguousarray(r, dtype=np.float32)
    with np.errstate(all='ignore'):
        v = g + r
        assert v.dtype == np.float32
        w = narrow(wire_dt, v)
        wf = widen(wire_dt, w)
        rn = np.where(np.isfinite(wf), v - wf, np.float32(0)).astype(np.float32)
    return w, rn


def step_or_cast(wire_dt, g, r):
    """`step` where there is a residual, the plain cast where r is None: (w, r' or None)."""
    return step(wire_dt, g, r) if r is not None else (narrow(wire_dt, g), None)


def reduce_ref(oracle, wire_dt, ws, plan_wire_bytes, op, P):
    """The contract's result for one segment from the ranks' WIRE values (rank order)."""
    out = widen(wire_dt, oracle.fold_ref_order(wire_dt, ws, plan_wire_bytes))
    if op == OP_AVG:
        with np.errstate(all='ignore'):
            out = (out / np.float32(P)).astype(np.float32)
    return out


def constant_sequence(wire_dt, value, steps):
    """A constant gradient from residual 0: the widened wire value of every step, the last residual."""
    g, r, seen = np.array([value], np.float32), np.zeros(1, np.float32), []
    for _ in range(steps):
        w, r = step(wire_dt, g, r)
        seen.append(float(widen(wire_dt, w)[0]))
    return seen, float(r[0])


def test_cpu_model_values():
    """The values the issue pins (run as part of the CPU suite by tests/test_feedback_mirror_cpu.py)."""
    z = np.zeros(SPECIALS.size, np.float32)
    w, r = step(DT_BFLOAT16, SPECIALS, z)
    assert r.tolist() == [1, 3, -17, -16, 160, -1.1717737891103752e-11, -2.3216983890961274e-12,
                          -3.5154101851730957e-11, 0, 0, 0, 2.0 ** -8, -2.0 ** -8, 0]
    wf = widen(DT_BFLOAT16, w)
    assert wf[:5].tolist() == [2048, 2048, 65536, 65536, 99840]
    assert wf[8] == 0 and not np.signbit(wf[8])  # -0.0 + 0 is +0.0
    assert np.isnan(wf[9]) and wf[10] == -np.inf and wf[11:].tolist() == [1.0, 1.015625, np.inf]
    w, r = step(DT_HALF, SPECIALS, z)
    f = np.float32
    assert r.tolist() == [1, -1, 15, 0, 0, float(f(1e-8)), float(f(2.98e-8)), float(f(3.0e-8) - f(2.0 ** -24)),
                          0, 0, 0, 0, 0, 0]
    assert constant_sequence(DT_BFLOAT16, 1 + 2.0 ** -10, 8) == ([1, 1, 1, 1, 1.0078125, 1, 1, 1], 0.0)
    assert constant_sequence(DT_HALF, 1 + 2.0 ** -13, 8) == ([1, 1, 1, 1, 1.0009765625, 1, 1, 1], 0.0)
    # the sum of what was sent equals the sum of the true values
    seen, _ = constant_sequence(DT_BFLOAT16, 1 + 2.0 ** -10, 8)
    assert sum(seen) == 8 * (1 + 2.0 ** -10)
    # an fp16 gradient of 1e-8 is carried whole in the residual until it reaches the wire
    seen, _ = constant_sequence(DT_HALF, 1e-8, 8)
    assert seen[:2] == [0.0, 0.0] and any(s > 0 for s in seen)
