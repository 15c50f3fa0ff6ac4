"""The NumPy model of the scale factors (_scale_helpers) on the values the contract names, and the
Python-side argument validation, as far as it runs without a GPU."""
import numpy as np
import pytest
import torch

from _helpers import DT_BFLOAT16, DT_HALF
from _scale_helpers import FACTORS, OP_AVG, OP_SUM, mul, pack_feedback, result, same_bits, scale_input, special_values
from _wire_helpers import narrow, widen

F = np.finfo(np.float32)


def test_one_is_absent():
    """a == 1: the bits are untouched, a NaN's payload included."""
    x = np.array([0x7fc12345, 0xffc00001, 0x00000001, 0x80000000], np.uint32).view(np.float32)
    assert mul(x, 1.0).view(np.uint32).tolist() == x.view(np.uint32).tolist()
    assert result(x, OP_SUM, 3, 1.0).view(np.uint32).tolist() == x.view(np.uint32).tolist()


def test_subnormal_products_are_kept():
    """A product in the subnormal range is the correctly rounded subnormal, not zero."""
    y = mul(np.array([F.tiny, F.tiny * 3, -F.tiny], np.float32), 0.5)
    assert y.tolist() == [2.0 ** -127, 3 * 2.0 ** -127, -2.0 ** -127] and (y != 0).all()
    # 2^-149 is the smallest subnormal: half of it ties to even (zero), three halves to 2 * 2^-149
    y = mul(np.array([F.smallest_subnormal, 3 * F.smallest_subnormal], np.float32), 0.5)
    assert y.tolist() == [0.0, 2 * 2.0 ** -149]
    # a subnormal input scaled up is exact
    assert mul(np.array([F.smallest_subnormal], np.float32), 3.0).tolist() == [3 * 2.0 ** -149]
    y = mul(np.array([1.0], np.float32), 2.0 ** -16) * np.float32(2.0 ** -120)
    assert y[0] == np.float32(2.0 ** -136)


def test_overflow_gives_inf_and_specials_stay():
    y = mul(np.array([F.max, -F.max, F.max / 3, np.inf, -np.inf, 0.0, -0.0], np.float32), 3.0)
    assert y[:2].tolist() == [np.inf, -np.inf] and np.isfinite(y[2])
    assert y[3:5].tolist() == [np.inf, -np.inf]
    assert y[5] == 0 and not np.signbit(y[5]) and y[6] == 0 and np.signbit(y[6])
    assert np.isnan(mul(np.array([np.nan], np.float32), 0.5)[0])
    assert np.isnan(result(np.array([np.nan], np.float32), OP_AVG, 3, 0.5)[0])


def test_quotient_then_factor():
    """AVG with a postscale is (s / P) * b with both roundings, not s * (b / P) and not (s * b) / P."""
    rng = np.random.default_rng(5)
    s = rng.standard_normal(20000).astype(np.float32)
    b = np.float32(1.0 / 3.0)
    want = ((s / np.float32(3)).astype(np.float32) * b).astype(np.float32)
    got = result(s, OP_AVG, 3, b)
    assert got.tobytes() == want.tobytes()
    other = ((s * b).astype(np.float32) / np.float32(3)).astype(np.float32)
    fused = (s * np.float32(b / np.float32(3))).astype(np.float32)
    assert (got != other).any() and (got != fused).any()  # the order is observable
    # SUM, and AVG at P = 1: the factor alone
    assert result(s, OP_SUM, 3, b).tobytes() == (s * b).astype(np.float32).tobytes()
    assert result(s, OP_AVG, 1, b).tobytes() == (s * b).astype(np.float32).tobytes()
    # a quotient that lands in the subnormal range is rounded there before the factor is applied
    t = np.array([F.tiny, 5 * F.smallest_subnormal], np.float32)
    assert result(t, OP_AVG, 3, 3.0).tolist() == [float(np.float32(F.tiny / np.float32(3)) * np.float32(3)),
                                                  float(np.float32(2 * F.smallest_subnormal) * np.float32(3))]


def test_product_never_fuses_with_the_feedback_sum():
    """v = (g (x) a) (+) r with two roundings: an fma of g, a and r gives other bits for some inputs."""
    rng = np.random.default_rng(11)
    g = rng.standard_normal(50000).astype(np.float32)
    r = (rng.standard_normal(50000) * 2.0 ** -10).astype(np.float32)
    a = np.float32(1.0 / 3.0)
    w, rn = pack_feedback(DT_BFLOAT16, g, r, a)
    v = ((g * a).astype(np.float32) + r).astype(np.float32)
    assert widen(DT_BFLOAT16, w).tobytes() == widen(DT_BFLOAT16, narrow(DT_BFLOAT16, v)).tobytes()
    assert rn.tobytes() == (v - widen(DT_BFLOAT16, w)).astype(np.float32).tobytes()
    fma = (g.astype(np.float64) * np.float64(a) + r.astype(np.float64)).astype(np.float32)  # one rounding (exact in fp64)
    assert (fma != v).any()


def test_the_motivating_case():
    """Two ranks hold 40000: their fp16 sum is inf; with prescale 0.5 it is exactly 40000."""
    g = np.array([40000.0], np.float32)
    w = narrow(DT_HALF, g)
    with np.errstate(all='ignore'):
        assert np.isinf(widen(DT_HALF, (w + w).astype(np.float16)))[0]
    h = narrow(DT_HALF, mul(g, 0.5))
    s = widen(DT_HALF, (h + h).astype(np.float16))
    assert result(s, OP_SUM, 2, 1.0).tolist() == [40000.0]
    assert result(s, OP_AVG, 2, 2.0).tolist() == [40000.0]


def test_helpers_inputs():
    for a in FACTORS:
        s = special_values(a)
        with np.errstate(all='ignore'):
            y = mul(s, a)
        assert np.isnan(s).any() and np.isinf(s).any() and (s == 0).any()
        if a > 1:
            assert (np.isinf(y) & np.isfinite(s)).any(), 'no product overflows'
        if a < 1:
            assert ((y != 0) & (np.abs(y) < F.tiny) & (np.abs(s) >= F.tiny)).any(), 'no product lands in the subnormals'
        x = scale_input(300, 3, a)
        assert same_bits(x[:s.size], s) and same_bits(x, x.copy()) and not same_bits(x, -x)


def test_python_argument_validation():
    """A factor on a tensor the engine cannot scale, with MIN / MAX, or a bad factor: ValueError before
    anything is submitted (no communicator exists here, so a submission would fail differently)."""
    from ddl.torch import cpp_backend as cb
    from ddl.torch import tensor_communicate as tc
    assert cb.SCALE == 0x4000
    import ctypes
    assert ctypes.sizeof(cb.ScaleArg) == 24 and cb.ScaleArg.prescale.offset == 16 and cb.ScaleArg.postscale.offset == 20
    assert cb.ScaleArg.user.offset == cb.SumsqArg.user.offset and cb.ScaleArg.sumsq.offset == cb.SumsqArg.sumsq.offset
    t = torch.zeros(8)
    for kw in ({'prescale': 0.5}, {'postscale': 2.0}):
        with pytest.raises(ValueError, match='device'):
            tc.allreduce_async(t, 'k', **kw)
        with pytest.raises(ValueError, match='device'):
            tc.allreduce_async_batch([t, t], ['a', 'b'], **kw)
        with pytest.raises(ValueError, match='OP_MIN'):
            tc.allreduce_async(t, 'k', op=cb.OP_MAX, **kw)
        with pytest.raises(ValueError, match='OP_MIN'):
            tc.allreduce_async_batch([t], ['a'], op=cb.OP_MIN, **kw)
    for bad in (0.0, -1.0, float('inf'), float('nan'), 1e39, 1e-46):
        with pytest.raises(ValueError, match='scale factor'):
            tc.allreduce_async(t, 'k', prescale=bad)
        with pytest.raises(ValueError, match='scale factor'):
            tc.allreduce_async(t, 'k', postscale=bad)
        with pytest.raises(ValueError, match='scale factor'):
            tc.allreduce_async_batch([t, t], ['a', 'b'], postscale=[1.0, bad])
    with pytest.raises(ValueError, match='one per tensor'):
        tc.allreduce_async_batch([t, t], ['a', 'b'], prescale=[0.5])
    with pytest.raises(ValueError, match='device'):  # per tensor: only the scaled ones are checked
        tc.allreduce_async_batch([t, t], ['a', 'b'], prescale=[1.0, 0.5])
    sp = torch.zeros(4, 4).to_sparse()
    with pytest.raises(ValueError):
        tc.allreduce_async(sp, 'k', prescale=0.5)


def test_wrapper_arguments():
    from ddl.torch.parallelism.data import DynamicLossScaler, data_parallelism_distributed_optimizer_wrapper
    m = torch.nn.Linear(3, 2)
    base = torch.optim.SGD(m.parameters(), lr=0.1)
    for bad in (0.0, -2.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='gradient_predivide_factor'):
            data_parallelism_distributed_optimizer_wrapper(base, gradient_predivide_factor=bad)
    opt = data_parallelism_distributed_optimizer_wrapper(base, gradient_predivide_factor=4)
    assert opt.gradient_predivide_factor == 4.0 and opt.loss_scale == 1.0 and not opt.skip_nonfinite
    cpu = torch.zeros(3)
    assert opt._engine_factors(cpu) == (1.0, 1.0)
    with pytest.raises(TypeError):
        DynamicLossScaler(base)
    with pytest.raises(ValueError):
        DynamicLossScaler(opt, init_scale=0.0)
    sc = DynamicLossScaler(opt, init_scale=2.0 ** 10, growth_interval=2)
    assert opt.skip_nonfinite and opt.loss_scale == 1024.0
    loss = torch.tensor(3.0)
    assert sc.scale(loss).item() == 3072.0
