"""Error feedback of the e4m3 wire (DDL_ALLREDUCE_WIRE_E4M3_FEEDBACK; include/ddl_amd.h "Error feedback of the e4m3
wire") restated on the CPU on top of _e4m3_helpers, bit for bit. Never the engine's own output.

Per granule of a request with a residual r (fp32, indexed like the tensor, zero the first time), all in fp32, every
operation rounded on its own:
    c  = g, or g * prescale
    v  = c + r
    (codes, s) = the plain pack's rule over the granule's v
    d  = code * s
    r' = isfinite(v - d) ? v - d : +0.0
(not finite: v is a NaN or an infinity — d is a NaN then — or v is finite and past 248 * 2**120, whose code 256 and up
under the largest scale 2**120 decodes to an infinity in fp32).
Only the pack's quantization is compensated: the fold requantizes the sum as it does without the bit.
"""
import numpy as np

import _e4m3_helpers as q8

F = np.float32
WIRE_E4M3_FEEDBACK = 0x40000  # enum ddl_allreduce_wire8_feedback
G = q8.G


def pack_fb(g, r, prescale=1.0):
    """One request's fp32 tensor g and residual r (same size) -> (its granules, the new residual)."""
    g = np.ascontiguousarray(g, F).ravel()
    r = np.ascontiguousarray(r, F).ravel()
    assert g.size == r.size
    with np.errstate(all='ignore'):
        c = (g * F(prescale)).astype(F) if prescale != 1.0 else g
        v = (c + r).astype(F)
        wire = q8.quantize(v)
        d = q8.dequantize(wire)[:v.size]
        e = (v - d).astype(F)
        rn = np.where(np.isfinite(e), e, F(0)).astype(F)
    return wire, rn


def half_quantum(wire, n):
    """Per element, the largest |v - d| the rule allows for a finite v that was sent as this code: half the distance
    between the code and its neighbour away from zero (the grid is finer towards zero), times the granule's scale;
    0 -> half the smallest subnormal code. fp64."""
    w = np.ascontiguousarray(wire, np.uint8).reshape(-1, q8.GRANULE)
    s = w[:, G:].copy().view(F).astype(np.float64)
    e = ((w[:, :G] >> 3) & 15).astype(np.int64)
    step = np.ldexp(1.0, np.maximum(e, 1) - 7 - 3)  # spacing of the codes of this exponent (subnormals: 2**-9)
    return (0.5 * step * s[:, None]).ravel()[:n]


def allreduce_steps(xs_per_step, op=q8.OP_SUM, prescale=1.0, postscale=1.0, residuals=None, feedback=None):
    """Consecutive steps of one request under one name: xs_per_step[t][r] is rank r's tensor at step t. residuals[r]:
    rank r's residual before the first step (None: zeros). feedback[r]: whether rank r carries the bit (None: all).
    Returns (the outputs per step, the ranks' residuals after the last step)."""
    P, n = len(xs_per_step[0]), xs_per_step[0][0].size
    res = [np.zeros(n, F) if residuals is None or residuals[r] is None else np.array(residuals[r], F) for r in range(P)]
    outs = []
    for xs in xs_per_step:
        wires = []
        for r in range(P):
            if feedback is None or feedback[r]:
                w, res[r] = pack_fb(xs[r], res[r], prescale)
            else:
                w = q8.pack(xs[r], prescale)
            wires.append(w)
        total = q8.fold(wires) if P > 1 else wires[0]
        outs.append(q8.unpack(total, n, op, P, postscale))
    return outs, res


def residual_seed(n, seed):
    """A residual as a previous step leaves it: what pack_fb removes from another seeded input of the same size."""
    return pack_fb(q8.rank_input(n, seed + 500), np.zeros(n, F))[1]


def step_inputs(P, lens, seed, step):
    """xs[r][i] of step `step` of the engine tests: _e4m3_helpers.engine_inputs with another seed per step, and the
    NaNs and infinities (rank 0) at the even steps only, so that the step behind them shows whether a residual
    survived one."""
    return [[q8.rank_input(n, seed + 17 * i + 1000 * step, r, specials=step % 2 == 0) for i, n in enumerate(lens)]
            for r in range(P)]
