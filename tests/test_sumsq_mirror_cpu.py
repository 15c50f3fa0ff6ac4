"""The NumPy restatement of the engine's sum of squares (_sumsq_helpers.mirror; include/ddl_amd.h "Sum
of squares") against exact arithmetic, and the torch mirror's refusals of `sumsq=True` — no GPU.

Bound: the squares of fp32 values are exact in fp64, and for n non-negative terms every summation
order stays within relative (n-1) u / (1 - (n-1) u) of the exact sum, u = 2^-53 (Higham, Accuracy and
Stability of Numerical Algorithms, section 4.2)."""
import math
import struct

import numpy as np
import pytest
import torch

from _sumsq_helpers import exact_bound, mirror


def _bits(v):
    return struct.pack('<d', v)


@pytest.mark.parametrize('compressed', [False, True], ids=['fp32', 'wire'])
@pytest.mark.parametrize('n', [1, 4, 257, 16385, 70_001])
def test_mirror_within_the_bound_of_the_exact_sum(n, compressed):
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)).astype(np.float32)
    exact = math.fsum(float(v) * float(v) for v in x.astype(np.float64))  # every product exact, fsum exactly rounded
    for cuts in ((), (n // 3 // 64 * 64, n // 2 // 64 * 64)):
        got = mirror(x, compressed, cuts)
        # + 2^-53: fsum's own rounding of the exact sum
        assert abs(got - exact) <= (exact_bound(n) + 2.0 ** -53) * exact, (n, cuts, got, exact)
    if n == 1:
        assert _bits(mirror(x, compressed)) == _bits(float(x[0]) * float(x[0]))


def test_order_is_the_documented_one():
    """A case small enough to write down: 5 elements, one tile; lane 0 owns elements 0..3 and lane 1
    element 4 (uncompressed), lane 0 owns all five (compressed)."""
    x = np.array([1.0, 2.0 ** -30, 2.0 ** -30, 2.0 ** 27, 3.0], np.float32)
    sq = [float(v) ** 2 for v in x]
    lane0 = ((sq[0] + sq[1]) + sq[2]) + sq[3]
    assert _bits(mirror(x, False)) == _bits(lane0 + sq[4])
    assert _bits(mirror(x, True)) == _bits(lane0 + sq[4])
    # a cut makes two pieces, added in offset order from the first piece's value
    assert _bits(mirror(x, False, cuts=(4,))) == _bits(lane0 + sq[4])
    y = np.arange(1, 600, dtype=np.float32)
    assert mirror(y, False) == float(np.sum(y.astype(np.float64) ** 2))  # small integers: every order is exact
    assert mirror(y, True, cuts=(256,)) == mirror(y, False)


def test_special_values():
    f = np.float32
    assert _bits(mirror(np.zeros(0, f), False)) == _bits(0.0)
    assert _bits(mirror(np.array([-0.0, -0.0, 0.0], f), True)) == _bits(0.0)
    assert mirror(np.array([1.0, np.inf, 2.0], f), False) == math.inf
    assert mirror(np.array([-np.inf], f), False) == math.inf
    assert math.isnan(mirror(np.array([1.0, np.nan], f), False))
    assert math.isnan(mirror(np.array([np.inf, 1.0, np.nan], f), True))
    big = mirror(np.full(5000, np.finfo(f).max, f), False)
    assert math.isfinite(big) and big > 1e80
    sub = np.finfo(f).smallest_subnormal
    assert mirror(np.array([sub], f), False) == float(sub) ** 2 > 0.0


def test_sumsq_refusals_raise_before_any_library_call(monkeypatch):
    """sumsq=True on a CPU tensor, on an fp16 tensor and with OP_MIN / OP_MAX: ValueError, and the
    library is never asked for anything."""
    from ddl.torch import cpp_backend as cb
    from ddl.torch import tensor_communicate as tc

    def boom(*a, **k):
        raise AssertionError('the library was called')
    monkeypatch.setattr(cb.CPPBackend, 'c_api', staticmethod(boom))
    monkeypatch.setattr(tc, '_comm', boom)
    cpu32, cpu16 = torch.zeros(8), torch.zeros(8, dtype=torch.float16)
    with pytest.raises(ValueError, match='device'):
        tc.allreduce_async(cpu32, 'a', sumsq=True)
    with pytest.raises(ValueError):
        tc.allreduce_async(cpu16, 'b', sumsq=True)
    with pytest.raises(ValueError, match='OP_MIN'):
        tc.allreduce_async(cpu32, 'c', op=cb.OP_MIN, sumsq=True)
    with pytest.raises(ValueError, match='OP_MIN'):
        tc.allreduce_async(cpu32, 'c', op=cb.OP_MAX, sumsq=True)
    with pytest.raises(ValueError, match='device'):
        tc.allreduce_async_batch([cpu32], ['d'], sumsq=True)
    with pytest.raises(ValueError):
        tc.allreduce_async_batch([cpu32, cpu16], ['e', 'f'], sumsq=[False, True])
    with pytest.raises(ValueError, match='OP_MIN'):
        tc.allreduce_async_batch([cpu32], ['g'], op=cb.OP_MAX, sumsq=[True])
    with pytest.raises(ValueError, match='one flag per tensor'):
        tc.allreduce_async_batch([cpu32], ['h'], sumsq=[True, False])
    # the dtype rule on its own (a stand-in for a device tensor: nothing is dereferenced)
    with pytest.raises(ValueError, match='float32'):
        tc._check_sumsq([_FakeCuda(torch.float16)], cb.OP_SUM, 'x')
    tc._check_sumsq([_FakeCuda(torch.float32)], cb.OP_AVG, 'x')


class _FakeCuda:
    """What _check_sumsq looks at of a dense device tensor."""
    is_sparse, is_cuda = False, True

    def __init__(self, dtype):
        self.dtype, self.device = dtype, torch.device('cpu')


def test_wrapper_norm_and_clip_at_size_one(monkeypatch):
    """At size 1 nothing is communicated; the wrapper reports torch's norm, clips by clip_grad_norm_'s
    rule and skips a step with a non-finite gradient."""
    from ddl.torch.parallelism.data import distributed_optimizer as do

    class One:
        size, rank, id = 1, 0, 0

    def make(**kw):
        torch.manual_seed(3)
        model = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Tanh(), torch.nn.Linear(5, 2))
        opt = do.data_parallelism_distributed_optimizer_wrapper(torch.optim.SGD(model.parameters(), lr=0.1),
                                                                communicator=One(), **kw)
        model(torch.ones(4, 7)).pow(2).sum().backward()
        return model, opt

    model, opt = make(track_grad_norm=True)
    grads = [p.grad.clone() for p in model.parameters()]
    want = math.sqrt(math.fsum(g.double().pow(2).sum().item() for g in grads))
    opt.step()
    assert opt.grad_norm == want and opt.found_nonfinite is False
    for p, g in zip(model.parameters(), grads):
        assert torch.equal(p.grad, g)  # tracking alone changes no gradient

    model, opt = make(max_grad_norm=want / 4)
    ref = [p.grad.clone().requires_grad_(False) for p in model.parameters()]
    holders = [torch.nn.Parameter(torch.zeros_like(g)) for g in ref]
    for h, g in zip(holders, ref):
        h.grad = g
    torch.nn.utils.clip_grad_norm_(holders, want / 4)
    opt.allreduce_gradients()
    assert opt.grad_norm == want
    for p, h in zip(model.parameters(), holders):
        torch.testing.assert_close(p.grad, h.grad)

    model, opt = make(skip_nonfinite=True)
    before = [p.detach().clone() for p in model.parameters()]
    next(iter(model.parameters())).grad[0, 0] = math.inf
    assert opt.step() is None and opt.found_nonfinite and opt.grad_norm == math.inf
    for p, b in zip(model.parameters(), before):
        assert torch.equal(p.detach(), b)
    model.zero_grad()
    model(torch.ones(4, 7)).pow(2).sum().backward()
    opt.step()
    assert not opt.found_nonfinite and not all(torch.equal(p.detach(), b) for p, b in zip(model.parameters(), before))
