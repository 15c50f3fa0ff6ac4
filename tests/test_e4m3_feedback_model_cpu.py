"""Error feedback of the e4m3 wire (DDL_ALLREDUCE_WIRE_E4M3_FEEDBACK) without a GPU: worked values of the rule, the
exactness of v - d against fp64, the property the feature exists for (nothing small is lost), wrong engines that must
each differ from the model of tests/_e4m3_feedback_helpers.py on the GPU tests' own inputs, and the constants and the
Python surface."""
import os
import re

import numpy as np
import pytest
import torch

import _e4m3_feedback_helpers as fb
import _e4m3_helpers as q8
from test_wire_mirror_cpu import _Comm, _Solo, device_kind, recorder  # noqa: F401 (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
Q, QF = 0x20000, 0x40000


def test_worked_values_of_the_rule():
    neg_nan = np.array([0xffc00000], np.uint32).view(F)[0]
    g = np.zeros(252, F)
    g[:6] = [448, 1.03, 2.0 ** -12, np.nan, -np.inf, neg_nan]
    w, r = fb.pack_fb(g, np.zeros(252, F))
    assert w[252:].copy().view(F)[0] == 1.0  # amax 448: s = 1
    assert w[1] == 0x38 and q8.DECODE[w[1]] == 1.0 and r[1] == F(1.03) - F(1.0) and r[1] == F(F(1.03) - 1)
    assert w[2] == 0 and r[2] == F(2.0 ** -12)  # below half the smallest code: all of it is kept
    assert w[3:6].tolist() == [0x7f, 0xff, 0xff] and r[3:6].tobytes() == np.zeros(3, F).tobytes()  # +0.0, not a NaN
    assert r[0] == 0 and not r[6:].any()
    # the next steps: the kept 2**-12 is added back, step after step, until it registers: v = 2, 3, 4 (a tie, to the
    # even code 0), 5 times 2**-12 -> 2**-9 = 8 x 2**-12 is sent and -3 x 2**-12 kept, which the next three steps use up
    sent = []
    for _ in range(8):
        w, r = fb.pack_fb(g, r)
        sent.append(q8.dequantize(w)[2])
    assert sent == [0, 0, 0, 2.0 ** -9, 0, 0, 0, 0] and r[2] == F(2.0 ** -12) and r[3:6].tobytes() == np.zeros(3, F).tobytes()
    # elements past n have no residual and stay +0.0 on the wire
    w, r = fb.pack_fb(np.array([3.0, 1.03], F), np.array([0.25, 0.5], F))
    assert r.size == 2 and not w[2:252].any()
    # the residual is in prescaled units
    third = F(1) / F(3)
    w, r = fb.pack_fb(np.array([448 * 3, 3.09], F), np.zeros(2, F), float(third))
    v = F(F(3.09) * third)
    assert r[1] == F(v - q8.dequantize(w)[1])


def _granule_zoo():
    rng = np.random.default_rng(5)
    zoo = []
    for e in (-149, -140, -126, -100, -8, 0, 8, 100, 119):  # fp32 subnormals up to the largest scale
        zoo.append(np.ldexp(rng.standard_normal(4 * 252), e).astype(F))
    for k in (-120, -3, 0, 60):
        for top in (448, 449, 1.75, 1.76):
            x = np.ldexp(rng.uniform(-1, 1, 252) * top, k).astype(F)
            x[7] = np.ldexp(F(top), k)
            zoo.append(x)
    for n, seed in ((20_011, 1), (1009, 2), (253, 3)):
        zoo.append(q8.rank_input(n, seed))  # every special of the GPU tests' inputs
    return zoo


def test_v_minus_d_is_exact():
    """For finite v the fp32 subtraction equals the fp64 one (so the rule costs one fp32 rounding, c + r, beyond the
    wire's own), and |r'| <= |v|; also from a non-zero residual."""
    for x in _granule_zoo():
        r = np.zeros(x.size, F)
        for _ in range(3):
            with np.errstate(all='ignore'):
                v = (x + r).astype(F)
            w, rn = fb.pack_fb(x, r)
            d = q8.dequantize(w)[:x.size]
            fin = np.isfinite(v)
            exact = v[fin].astype(np.float64) - d[fin].astype(np.float64)
            assert np.array_equal(rn[fin].astype(np.float64), exact)
            assert (np.abs(rn[fin]) <= np.abs(v[fin])).all()
            assert rn[~fin].tobytes() == np.zeros((~fin).sum(), F).tobytes() and np.isfinite(rn).all()
            r = rn


def test_nothing_small_is_lost():
    """A constant granule whose elements span 2**-12 .. 1 of its amax, K = 64 steps. With feedback
    sum_t d_t = K g - r_K up to the K roundings of c + r (each at most half an ulp of v), and |r_K| is at most one
    step's quantization error: half the code spacing at the element's code (the restatement computes it from the wire
    of every step). The plain pack misses that bound: an element below 2**-10 of amax is zero every step."""
    K = 64
    g = np.ldexp(F(1.37), -np.arange(252) % 13).astype(F) * np.where(np.arange(252) % 2, F(-1), F(1))
    g[0] = 1.75  # amax; the smallest elements are 1.37 * 2**-12
    assert np.abs(g).min() < 2.0 ** -11 * np.abs(g).max()
    r = np.zeros(252, F)
    sent, bound, vmax = np.zeros(252), np.zeros(252), np.zeros(252)
    for _ in range(K):
        with np.errstate(all='ignore'):
            vmax = np.maximum(vmax, np.abs((g + r).astype(F)).astype(np.float64))
        w, r = fb.pack_fb(g, r)
        sent += q8.dequantize(w)[:252].astype(np.float64)
        bound = np.maximum(bound, fb.half_quantum(w, 252))
    bound = bound + K * vmax * 2.0 ** -24
    err = np.abs(sent - K * g.astype(np.float64))
    assert (err <= bound).all(), (err / bound).max()
    plain = K * q8.dequantize(q8.pack(g))[:252].astype(np.float64)
    plain_bound = fb.half_quantum(q8.pack(g), 252) + K * np.abs(g).astype(np.float64) * 2.0 ** -24
    assert (np.abs(plain - K * g.astype(np.float64)) > plain_bound).any()  # the feature does something


# ---- wrong engines: each must differ from the model on the GPU tests' own inputs ---------------------------------
def _quantize_scale_from(v, c, saturate):
    """v quantized with the scale chosen from c. A quotient above 448 saturates, or overflows as the cast does."""
    n = v.size
    ng = q8.granules(n)
    pad = lambda a: np.concatenate([a, np.zeros(ng * 252 - n, F)]).reshape(ng, 252)  # noqa: E731
    x, cc = pad(v), pad(c)
    fin = np.isfinite(x)
    with np.errstate(all='ignore'):
        s = q8.scale_of(np.where(np.isfinite(cc), np.abs(cc), F(0)).max(axis=1).astype(F))
        y = (np.where(fin, x, F(0)) / s[:, None]).astype(F)
    if saturate:
        codes = q8.rne_codes(np.clip(y, -448, 448).ravel()).reshape(ng, 252).copy()
    else:
        codes = torch.from_numpy(y.ravel().copy()).to(torch.float8_e4m3fn).view(torch.uint8).numpy().reshape(ng, 252).copy()
    codes[~fin] = 0x7f | ((x.view(np.uint32) >> 24).astype(np.uint8) & 0x80)[~fin]
    out = np.zeros((ng, 256), np.uint8)
    out[:, :252] = codes
    out[:, 252:] = s.view(np.uint8).reshape(ng, 4)
    return out.ravel()


def _wrong_pack(kind):
    def pack(g, r, prescale=1.0):
        with np.errstate(all='ignore'):
            c = (g * F(prescale)).astype(F) if prescale != 1.0 else g
            v = (c + r).astype(F)
            if kind == 'residual behind the scale choice':  # the scale from c, v saturating into it
                w = _quantize_scale_from(v, c, True)
            elif kind == 'amax over c':  # the same scale, the conversion left to overflow
                w = _quantize_scale_from(v, c, False)
            else:
                w = q8.quantize(v)
            d = q8.dequantize(w)[:v.size]
            keep = np.ones(v.size, bool) if kind == 'a residual for NaN' else np.isfinite(v)
            rn = np.where(keep, (v - d).astype(F), F(0)).astype(F)
        return w, rn
    return pack


def _pack_in_pieces(g, r, cuts, wire_offsets):
    """The request packed piece by piece as fusion_pipeline_bytes cuts it; wire_offsets: a piece's residual taken at
    its WIRE byte offset / 4 instead of at its first element (the wrong engine)."""
    r = r.copy()
    wires = []
    edges = [0] + list(cuts) + [g.size]
    for a, b in zip(edges[:-1], edges[1:]):
        ra = a // 252 * 64 if wire_offsets else a
        w, r[ra:ra + b - a] = fb.pack_fb(g[a:b], r[ra:ra + b - a])
        wires.append(w)
    return np.concatenate(wires), r


def _two_steps(P, pack):
    """Outputs of the second of two steps over ENGINE_LENS at P ranks: the step where a wrong residual shows."""
    outs = []
    for i, n in enumerate(q8.ENGINE_LENS):
        res = [np.zeros(n, F) for _ in range(P)]
        for step in range(2):
            xs = fb.step_inputs(P, q8.ENGINE_LENS, q8.ENGINE_SEED, step)
            wires = []
            for r in range(P):
                w, res[r] = pack(xs[r][i], res[r])
                wires.append(w)
        outs.append(q8.unpack(q8.fold(wires), n))
    return outs


def _differs(a, b):
    return any(x.tobytes() != y.tobytes() for x, y in zip(a, b))


def test_wrong_engines_differ_on_the_gpu_tests_inputs():
    for P in (2, 3):
        want = _two_steps(P, fb.pack_fb)
        for kind in ('residual behind the scale choice', 'amax over c', 'a residual for NaN'):
            assert _differs(want, _two_steps(P, _wrong_pack(kind))), kind
        assert not _differs(want, _two_steps(P, _wrong_pack('the rule')))  # (the comparison itself)
        assert _differs(want, _two_steps(P, q8_plain)), 'no feedback at all'
    # a cut piece's residual offset: the engine tests' pipeline of 4096 bytes cuts the longest request
    n = q8.ENGINE_LENS[-1]
    cuts = q8.subplan_cuts(q8.ENGINE_LENS, 4096)[-1]
    assert cuts
    g0, g1 = q8.rank_input(n, 3), q8.rank_input(n, 4)
    _, r_right = _pack_in_pieces(g0, np.zeros(n, F), cuts, False)
    _, r_wrong = _pack_in_pieces(g0, np.zeros(n, F), cuts, True)
    assert r_right.tobytes() == fb.pack_fb(g0, np.zeros(n, F))[1].tobytes()  # cuts at granules change nothing
    w_right, _ = _pack_in_pieces(g1, r_right, cuts, False)
    assert w_right.tobytes() == fb.pack_fb(g1, r_right)[0].tobytes()
    assert w_right.tobytes() != _pack_in_pieces(g1, r_wrong, cuts, True)[0].tobytes(), 'residual offset in wire bytes'


def q8_plain(g, r, prescale=1.0):
    return q8.pack(g, prescale), r


# ---- constants and the Python surface ------------------------------------------------------------------------------
def test_constants_and_python_surface():
    from ddl.torch import Compression, cpp_backend as cb
    from ddl.torch.compression import wire_flag
    import ddl.torch.compression as comp
    from ddl.torch import tensor_communicate as tc
    assert cb.WIRE_E4M3_FEEDBACK == fb.WIRE_E4M3_FEEDBACK == QF
    with open(os.path.join(ROOT, 'include', 'ddl_amd.h')) as fh:
        header = fh.read()
    assert re.search(r'enum ddl_allreduce_wire8_feedback\s*\{\s*DDL_ALLREDUCE_WIRE_E4M3_FEEDBACK\s*=\s*0x40000\s*\}', header)
    assert 'Error feedback of the e4m3 wire' in header and 'IS NOT' in header
    for other in (cb.WIRE_FP16, cb.WIRE_BF16, cb.WIRE_FEEDBACK, cb.WIRE_STOCHASTIC, cb.WIRE_E4M3, cb.SUMSQ, cb.SCALE,
                  0x80, 0x400, 0x800, 0x10000, 0xff):
        assert not QF & other  # a free bit
    k = Compression.fp8_feedback
    assert wire_flag(k) == k.flag == Q | QF and repr(k) == 'Compression.fp8_feedback'
    assert k.feedback and not k.stochastic and not Compression.fp8.feedback
    assert Compression.bf16_feedback.feedback and not Compression.bf16.feedback
    with pytest.raises(TypeError, match='fp8_feedback'):
        wire_flag('fp8_feedback')
    doc = comp.__doc__
    assert 'fp8_feedback' in doc and 'not' in doc and '13.0 bytes' in doc and 'reset_error_feedback' in doc
    assert 'fp8' in comp.reset_error_feedback.__doc__
    assert not any('e4m3' in n.lower() or 'fb' in n.lower().split('_') for n in cb.DEPLOYMENT_API)  # an op bit only
    with open(os.path.join(ROOT, 'experiment-distributed-deep-learning_amd', 'csrc', 'ddl_amd.map')) as fh:
        assert 'e4m3' not in fh.read()
    with pytest.raises(ValueError, match='fresh'):  # its names are fresh per call: one leaked residual per call
        tc.allreduce_gradient(torch.ones(3), _Comm(), compression=k)


def test_flag_reaches_the_engine_for_fp32_device_requests_only(recorder, device_kind, monkeypatch):  # noqa: F811
    from ddl.torch import Compression, cpp_backend as cb
    from ddl.torch.tensor_communicate import allreduce_async, allreduce_async_batch
    dev32, dev16, host32 = torch.ones(5), torch.ones(5, dtype=torch.float16), torch.ones(5)
    device_kind += [dev32, dev16]
    k = Compression.fp8_feedback
    for op in (cb.OP_SUM, cb.OP_AVG):
        allreduce_async(dev32, 'a', _Comm(), output=dev32, op=op, compression=k).wait(5)
        assert recorder.calls[-1] == {'keys': ['a'], 'dts': [cb.DT_FLOAT], 'op': op | Q | QF, 'mem': cb.MEMORY_DEVICE}
        allreduce_async(dev16, 'b', _Comm(), output=dev16, op=op, compression=k).wait(5)
        assert recorder.calls[-1]['op'] == op  # not fp32: no wire bit
        allreduce_async(host32, 'c', _Comm(), output=host32, op=op, compression=k).wait(5)
        assert recorder.calls[-1] == {'keys': ['c'], 'dts': [cb.DT_FLOAT], 'op': op, 'mem': cb.MEMORY_HOST}
    allreduce_async(dev32, 'a', _Solo(), output=dev32, compression=k).wait(5)
    assert recorder.calls[-1]['op'] == cb.OP_SUM  # size 1 with the shortcut: nothing is quantized, no residual
    del recorder.calls[:]
    ts = [dev32, dev16, host32]
    for h in allreduce_async_batch(ts, ['k0', 'k1', 'k2'], _Comm(), outputs=ts, op=cb.OP_AVG, compression=k):
        h.wait(5)
    assert sorted(c['op'] for c in recorder.calls) == [cb.OP_AVG, cb.OP_AVG, cb.OP_AVG | Q | QF]
    for op in (cb.OP_MIN, cb.OP_MAX):
        with pytest.raises(ValueError):
            allreduce_async(dev32, 'a', _Comm(), output=dev32, op=op, compression=k)


@pytest.mark.parametrize('overlap', [False, True])
def test_wrapper_carries_the_flag(recorder, device_kind, monkeypatch, overlap):  # noqa: F811
    from ddl.torch import Compression, cpp_backend as cb
    from ddl.torch import tensor_communicate as tc
    from ddl.torch.parallelism.data import data_parallelism_distributed_optimizer_wrapper
    monkeypatch.setattr(tc, 'memory_kind', lambda t, what='tensor': cb.MEMORY_DEVICE)
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Tanh(), torch.nn.Linear(5, 2))
    opt = data_parallelism_distributed_optimizer_wrapper(
        torch.optim.SGD(model.parameters(), lr=0.1), _Comm(), pin_host_gradients=False, fused_mean=True,
        compression=Compression.fp8_feedback, overlap_backward=overlap, bucket_bytes=None)
    names = []
    for _ in range(2):
        del recorder.calls[:]
        opt.zero_grad()
        model(torch.randn(4, 6)).sum().backward()  # (with overlap_backward the requests leave from here)
        opt.step()
        assert sum(len(c['keys']) for c in recorder.calls) == 4
        assert all(c['op'] == cb.OP_AVG | Q | QF for c in recorder.calls)
        names.append(sorted(key for c in recorder.calls for key in c['keys']))
    assert names[0] == names[1]  # stable names: the residuals are found again
