"""The block-scaled e4m3 wire (DDL_ALLREDUCE_WIRE_E4M3) without a GPU: the format's worked values, the scale rule
at its edges, the properties of the model of tests/_e4m3_helpers.py that the GPU tests compare against, wrong engines
that must each differ from it on those tests' own inputs, and the constants and the Python surface."""
import os
import re

import numpy as np
import pytest
import torch

import _e4m3_helpers as q8
from test_wire_mirror_cpu import _Comm, _Solo, device_kind, recorder  # noqa: F401 (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _scale(wire, g=0):
    return wire.reshape(-1, 256)[g, 252:].copy().view(np.float32)[0]


def test_worked_values_of_the_format():
    x = np.zeros(252, F)
    x[:7] = [448, 1, 17, 19, 21, 23, 2.0 ** -9]
    w = q8.pack(x)
    assert _scale(w) == 1.0
    assert q8.dequantize(w)[:8].tolist() == [448, 1, 16, 20, 20, 24, 2.0 ** -9, 0]  # ties to even, a subnormal code
    neg_nan = np.array([0xffc00000], np.uint32).view(F)[0]
    w = q8.pack(np.array([1, np.inf, neg_nan, 3], F))
    assert w[:4].tolist() == [0x70, 0x7f, 0xff, 0x7c] and w[252:].tolist() == [0x00, 0x00, 0x00, 0x3c]
    assert not w[4:252].any()  # elements past n: +0.0
    assert w.size == 256 and q8.pack(np.zeros(253, F)).size == 512 and q8.pack(np.zeros(0, F)).size == 0
    d = q8.dequantize(w)
    assert np.isnan(d[1]) and np.isnan(d[2]) and d[0] == 1 and d[3] == 3  # an infinity comes back as NaN


def test_scale_rule_at_its_edges():
    tiny = F(2.0 ** -126)
    for amax, s in [(0, tiny), (1e-45, tiny), (1e-39, tiny), (448 * 2.0 ** -126, tiny), (449 * 2.0 ** -126, 2 * tiny),
                    (448, 1), (449, 2), (np.nextafter(F(448), F(1000)), 2), (1.0, 2.0 ** -8), (1.75, 2.0 ** -8),
                    (1.76, 2.0 ** -7), (3.4e38, 2.0 ** 120), (3.4028235e38, 2.0 ** 120)]:
        got = q8.scale_of(F(amax))
        assert got == F(s), (amax, got, s)
        assert F(amax) / got <= 448 and (got == tiny or F(amax) / (got / 2) > 448)
    # the integer form the kernels use (csrc/e4m3.h scale_exponent) is the same rule
    rng = np.random.default_rng(1)
    u = np.concatenate([rng.integers(0, 0x7f800000, 200_000, dtype=np.uint32),
                        (np.arange(1, 255, dtype=np.uint32) << 23) | np.uint32(0x600000),
                        (np.arange(1, 255, dtype=np.uint32) << 23) | np.uint32(0x600001)])
    se = np.maximum(((u.astype(np.int64) + 0x1fffff) >> 23) - 8, 1).astype(np.uint32)
    assert np.array_equal((se << 23).view(F), q8.scale_of(u.view(F)))
    # amax is taken over the finite elements only
    w = q8.pack(np.array([1.0, np.inf, np.nan, -3.0], F))
    assert _scale(w) == F(2.0 ** -7)
    assert _scale(q8.pack(np.array([np.inf, np.nan], F))) == tiny


def _rne_integer(y):
    """RNE onto e4m3fn restated in integer arithmetic, |y| <= 448: an independent check of the model's quantizer."""
    u = np.ascontiguousarray(y, F).view(np.uint32)
    a, sign = u & 0x7fffffff, (u >> 24) & 0x80
    normal = (((a.astype(np.uint64) + 0x7ffff + ((a >> 20) & 1)) >> 20) - (120 << 3)).astype(np.int64)
    sub = np.rint(a.view(F).astype(np.float64) * 512.0).astype(np.int64)
    return (sign | np.where(a >= 0x3c800000, normal, sub)).astype(np.uint8)


def test_the_models_quantizer_is_rne_with_subnormals():
    d = q8.DECODE[:0x7f].astype(np.float64)
    mid = ((d[:-1] + d[1:]) / 2).astype(F)
    ys = np.concatenate([mid, np.nextafter(mid, F(0)), np.nextafter(mid, F(1000)), q8.DECODE[:0x7f],
                         np.random.default_rng(2).uniform(-448, 448, 100_000).astype(F),
                         np.ldexp(np.random.default_rng(3).standard_normal(100_000), -8).astype(F)])
    ys = np.concatenate([ys, -ys, np.array([0.0, -0.0, 1e-45, -1e-45], F)])
    ys = ys[np.abs(ys) <= 448]
    got = q8.rne_codes(ys)
    assert np.array_equal(got, _rne_integer(ys))
    # a tie goes to the even code, the codes themselves are fixed points, -0 and subnormal codes are kept
    assert np.array_equal(q8.rne_codes(mid), np.where(np.arange(126) % 2 == 0, np.arange(126), np.arange(126) + 1))
    assert np.array_equal(q8.rne_codes(q8.DECODE[:0x7f]), np.arange(0x7f))
    assert q8.rne_codes(np.array([-0.0, 2.0 ** -9, -3 * 2.0 ** -9], F)).tolist() == [0x80, 0x01, 0x83]


@pytest.mark.parametrize('P', q8.ENGINE_RANKS)
def test_requantizing_decoded_values_is_lossless(P):
    """dequant(quant(dequant(q))) == dequant(q): a P = 1 data plane, or a schedule that copies, changes no value —
    on packed contributions and on folded sums. (The bytes may change: a granule whose largest value rounded down
    may requantize under a smaller scale, onto the same values.)"""
    xs = q8.engine_inputs(P, q8.ENGINE_LENS, q8.ENGINE_SEED)
    for i in range(len(q8.ENGINE_LENS)):
        wires = [q8.pack(xs[r][i]) for r in range(P)]
        for w in wires[:2] + [q8.fold(wires)]:
            d = q8.dequantize(w)
            fin = np.isfinite(d)
            again = q8.dequantize(q8.quantize(d))
            assert np.array_equal(again[fin], d[fin]) and np.isnan(again[~fin]).all()


@pytest.mark.parametrize('P', [2, 3, 8])
def test_error_bound_on_random_data(P):
    """A contribution's error is below amax_granule / 14 (half the top binade's spacing is 16 s and s < amax / 224),
    the sum's second quantization adds less than amax(sum's granule) / 14."""
    n = 40 * q8.G
    xs = [q8.rank_input(n, 11, r, specials=False) for r in range(P)]
    exact = np.zeros(n, np.float64)
    budget = np.zeros(n, np.float64)
    deq = []
    for x in xs:
        d = q8.dequantize(q8.pack(x))
        amax = np.abs(x).reshape(-1, q8.G).max(axis=1).astype(np.float64)
        assert (np.abs(d.astype(np.float64) - x).reshape(-1, q8.G) <= (amax / 14)[:, None]).all()
        exact += x
        budget += np.repeat(amax / 14, q8.G)
        deq.append(d)
    got = q8.allreduce(xs).astype(np.float64)
    s32 = deq[0]
    for d in deq[1:]:
        s32 = (s32 + d).astype(F)
    budget += np.repeat(np.abs(s32).reshape(-1, q8.G).max(axis=1).astype(np.float64) / 14, q8.G)
    budget += P * np.abs(exact) * 2.0 ** -23  # the fp32 additions
    assert (np.abs(got - exact) <= budget).all()


# ---- wrong engines: each must differ from the model on the GPU tests' own inputs ---------------------------------
def _trunc_codes(y):
    y = np.ascontiguousarray(y, F)
    mag = np.abs(y).astype(np.float64)
    idx = np.searchsorted(q8.DECODE[:0x7f].astype(np.float64), mag, side='right') - 1
    return (idx.astype(np.uint8) | ((y.view(np.uint32) >> 24).astype(np.uint8) & 0x80)).astype(np.uint8)


def _mx_scale(amax):
    amax = np.asarray(amax, F)
    _, e = np.frexp(amax.astype(np.float64))  # amax = m 2**e, m in [0.5, 1): floor(log2 amax) = e - 1
    return np.ldexp(1.0, np.maximum(e - 1 - 8, -126)).astype(F)


def _saturating_rne(y):
    return q8.rne_codes(np.clip(y, -448, 448))


def _engine_results(P, **how):
    xs = q8.engine_inputs(P, q8.ENGINE_LENS, q8.ENGINE_SEED)
    return [how['run']([xs[r][i] for r in range(P)]) for i in range(len(q8.ENGINE_LENS))]


def _differs(a, b):
    return any(x.tobytes() != y.tobytes() for x, y in zip(a, b))


def test_wrong_engines_differ_on_the_gpu_tests_inputs():
    third = float(F(1) / F(3))

    def model(xs, **kw):
        return q8.allreduce(xs, **kw)

    def per_hop(xs):  # requantizing after every addition, as a ring would
        acc = q8.pack(xs[0])
        for x in xs[1:]:
            acc = q8.fold([acc, q8.pack(x)])
        return q8.unpack(acc, xs[0].size)

    def variant(**q):
        def run(xs):
            return q8.unpack(q8.fold([q8.pack(x, **q) for x in xs], **q), xs[0].size)
        return run

    def prescale_behind(xs):  # quantize g, multiply the decoded value
        with np.errstate(all='ignore'):
            ys = [(q8.dequantize(q8.pack(x)) * F(third)).astype(F) for x in xs]
            y = ys[0]
            for d in ys[1:]:
                y = (y + d).astype(F)
        return q8.unpack(q8.quantize(y), xs[0].size)

    def postscale_first(xs):  # (y * b) / P instead of (y / P) * b
        y = q8.unpack(q8.fold([q8.pack(x) for x in xs]), xs[0].size)
        with np.errstate(all='ignore'):
            return ((y * F(third)).astype(F) / F(len(xs))).astype(F)

    for P in (3, 8):
        want = _engine_results(P, run=model)
        assert _differs(want, _engine_results(P, run=per_hop)), 'requantizing per hop'
        assert _differs(want, _engine_results(P, run=variant(finite_amax=False))), 'amax over non-finite elements'
        assert _differs(want, _engine_results(P, run=variant(rne=_trunc_codes))), 'truncation'
        assert _differs(want, _engine_results(P, run=variant(scale=_mx_scale, rne=_saturating_rne))), 'the MX scale rule'
    scaled = _engine_results(3, run=lambda xs: model(xs, prescale=third))
    assert _differs(scaled, _engine_results(3, run=prescale_behind)), 'the prescale behind the quantization'
    avg = _engine_results(3, run=lambda xs: model(xs, op=q8.OP_AVG, postscale=third))
    assert _differs(avg, _engine_results(3, run=postscale_first)), 'the postscale ahead of the quotient'
    assert not _differs(want, _engine_results(8, run=model))  # (the comparison itself: the model equals itself)


# ---- constants and the Python surface ------------------------------------------------------------------------------
def test_constants_and_python_surface():
    from ddl.torch import Compression, cpp_backend as cb
    from ddl.torch.compression import wire_flag
    import ddl.torch.compression as comp
    assert cb.WIRE_E4M3 == q8.WIRE_E4M3 == 0x20000
    with open(os.path.join(ROOT, 'include', 'ddl_amd.h')) as fh:
        header = fh.read()
    assert re.search(r'enum ddl_allreduce_wire8\s*\{\s*DDL_ALLREDUCE_WIRE_E4M3\s*=\s*0x20000\s*\}', header)
    for other in (cb.WIRE_FP16, cb.WIRE_BF16, cb.WIRE_FEEDBACK, cb.WIRE_STOCHASTIC, cb.SUMSQ, cb.SCALE, 0x80, 0x400,
                  0x800, 0x10000, 0xff):
        assert not cb.WIRE_E4M3 & other  # a free bit
    k = Compression.fp8
    assert wire_flag(k) == k.flag == 0x20000 and repr(k) == 'Compression.fp8'
    assert not k.feedback and not k.stochastic
    with pytest.raises(TypeError, match='fp8'):
        wire_flag('fp8')
    assert 'fp8' in comp.__doc__ and 'e4m3' in comp.__doc__ and '16 ranks' in comp.__doc__
    assert not any('e4m3' in n.lower() for n in cb.DEPLOYMENT_API)  # the feature is an op bit


def test_flag_reaches_the_engine_for_fp32_device_requests_only(recorder, device_kind, monkeypatch):  # noqa: F811
    from ddl.torch import Compression, cpp_backend as cb
    from ddl.torch import tensor_communicate as tc
    from ddl.torch.tensor_communicate import allreduce_async, allreduce_async_batch
    dev32, dev16, host32 = torch.ones(5), torch.ones(5, dtype=torch.float16), torch.ones(5)
    device_kind += [dev32, dev16]
    k = Compression.fp8
    for op in (cb.OP_SUM, cb.OP_AVG):
        allreduce_async(dev32, 'a', _Comm(), output=dev32, op=op, compression=k).wait(5)
        assert recorder.calls[-1] == {'keys': ['a'], 'dts': [cb.DT_FLOAT], 'op': op | 0x20000, 'mem': cb.MEMORY_DEVICE}
        allreduce_async(dev16, 'b', _Comm(), output=dev16, op=op, compression=k).wait(5)
        assert recorder.calls[-1]['op'] == op  # not fp32: no wire bit
        allreduce_async(host32, 'c', _Comm(), output=host32, op=op, compression=k).wait(5)
        assert recorder.calls[-1] == {'keys': ['c'], 'dts': [cb.DT_FLOAT], 'op': op, 'mem': cb.MEMORY_HOST}
    allreduce_async(dev32, 'a', _Solo(), output=dev32, compression=k).wait(5)
    assert recorder.calls[-1]['op'] == cb.OP_SUM  # size 1 with the shortcut: nothing is quantized
    del recorder.calls[:]
    ts = [dev32, dev16, host32]
    for h in allreduce_async_batch(ts, ['k0', 'k1', 'k2'], _Comm(), outputs=ts, op=cb.OP_AVG, compression=k):
        h.wait(5)
    assert sorted(c['op'] for c in recorder.calls) == [cb.OP_AVG, cb.OP_AVG, cb.OP_AVG | 0x20000]
    for op in (cb.OP_MIN, cb.OP_MAX):
        with pytest.raises(ValueError):
            allreduce_async(dev32, 'a', _Comm(), output=dev32, op=op, compression=k)
    # allreduce_gradient takes it: no per-name state, so its fresh names are fine
    del recorder.calls[:]
    monkeypatch.setattr(tc, 'memory_kind', lambda t, what='tensor': cb.MEMORY_DEVICE)
    monkeypatch.setattr(tc, 'stream_handle_for', lambda t: 0)
    tc.allreduce_gradient(torch.ones(2, 3), _Comm(), fused_mean=True, compression=k)
    assert [c['op'] for c in recorder.calls] == [cb.OP_AVG | 0x20000]


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
        compression=Compression.fp8, overlap_backward=overlap, bucket_bytes=None)
    opt.zero_grad()
    model(torch.randn(4, 6)).sum().backward()
    opt.step()
    assert sum(len(c['keys']) for c in recorder.calls) == 4
    assert all(c['op'] == cb.OP_AVG | 0x20000 for c in recorder.calls)
