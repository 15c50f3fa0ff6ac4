"""The e4m3 wire over native bfloat16 tensors (include/ddl_amd.h "The e4m3 wire", the bfloat16 paragraph) restated on
the CPU from _e4m3_helpers.py and the widen / narrow of _bf16_native_helpers.py. Never the engine's own output. bf16
values are raw uint16.

    result = narrow(q8.unpack(q8.fold([q8.pack(widen(g_r), a) ...]), n, op, P, b))

The pack's product widen(g) (x) a is NOT narrowed; the unpack narrows once, behind the quotient and the postscale.
"""
import _e4m3_helpers as q8
from _bf16_native_helpers import rne, sumsq, wide  # noqa: F401  (sumsq: the 2-byte layout's order, re-exported)
from _helpers import DT_BFLOAT16  # noqa: F401


def pack(g, a=1.0):
    return q8.pack(wide(g), a)


def unpack(wire, n, op=q8.OP_SUM, P=1, b=1.0):
    return rne(q8.unpack(wire, n, op, P, b))


def allreduce(xs, op=q8.OP_SUM, a=1.0, b=1.0):
    """xs: the ranks' bf16 tensors in rank order. P = 1 with the data plane running: quantized once, no fold."""
    wires = [pack(x, a) for x in xs]
    return unpack(q8.fold(wires) if len(xs) > 1 else wires[0], xs[0].size, op, len(xs), b)


def rank_input(n, seed, rank=0, specials=True):
    """_e4m3_helpers.rank_input rounded to bf16: granules 2**40 apart, the specials on rank 0."""
    return rne(q8.rank_input(n, seed, rank, specials))


def engine_inputs(P, lens, seed):
    return [[rank_input(n, seed + 17 * i, r) for i, n in enumerate(lens)] for r in range(P)]
