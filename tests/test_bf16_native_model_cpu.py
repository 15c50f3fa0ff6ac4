"""The model of the native bfloat16 statistic and factors (_bf16_native_helpers.py) on the CPU: hand-worked
values, and wrong engines run in NumPy over all 65 536 patterns to show that the inputs the GPU tests use
(P = 3, the factors 1/3 and 3) reject them. Then the Python validation: bf16 accepted, float16 refused."""
import numpy as np
import pytest
import torch

import _bf16_native_helpers as bh
from _avg_helpers import quotient
from _bf16_native_helpers import ALL_BITS, OP_AVG, OP_SUM, THIRD, THREE, differing, mul, result, rne, wide
from _helpers import DT_BFLOAT16
from _sumsq_helpers import mirror


def _b(*patterns):
    return np.array(patterns, np.uint16)


def test_hand_worked_values():
    # widen: 0x3f80 = 1, 0x4040 = 3, 0x7f7f the largest finite value
    assert wide(_b(0x3f80, 0x4040, 0xc000)).tolist() == [1.0, 3.0, -2.0]
    # narrow, nearest even: 1 + 2^-8 is a tie and goes to the even 1.0, 1 + 3 * 2^-8 a tie that goes up to 1 + 2^-6
    assert rne(np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20], np.float32)).tolist() == \
        [0x3f80, 0x3f82, 0x3f81]
    assert rne(np.array([3.4e38, -3.4e38], np.float32)).tolist() == [0x7f80, 0xff80]  # overflow gives inf
    # pack: 1 (x) 1/3 = 0x3eaaaaab -> 0x3eab; 3 (x) 1/3 = 1 exactly in fp32; factor 1 moves the bytes, a signalling NaN included
    assert bh.pack(_b(0x3f80, 0x4040), THIRD).tolist() == [0x3eab, 0x3f80]
    assert bh.pack(_b(0x7f81, 0x0001), 1.0).tolist() == [0x7f81, 0x0001]
    # unpack, AVG at P = 3 with b = 3: (1 / 3) * 3 = 1 in fp32 (0x3eaaaaab * 3 rounds to 1), stored 0x3f80; a rounding
    # to bf16 between the two would give 0x3eab * 3 = 1.00195 -> 0x3f80 too, but 5: 5/3 = 0x3fd55555 * 3 = 5 -> 0x40a0
    # against 0x3fd5 * 3 = 4.9921875 -> 0x40a0 (tie-free, rounds up); the patterns that tell them apart are counted below
    assert bh.unpack(_b(0x3f80, 0x40a0), OP_AVG, 3, THREE).tolist() == [0x3f80, 0x40a0]
    # 7 / 3 * (1/3): fp32 2.3333333 * 0.33333334 = 0.7777778 -> 0x3f47; with a rounding between: 0x4015 = 2.328125,
    # * 1/3 = 0.7760417 -> 0x3f47 as well; 11: 3.6666667 / 3 = 1.2222223 -> 0x3f9c, between: 0x406b = 3.671875 / 3 -> 0x3f9d
    assert bh.unpack(_b(0x40e0, 0x4130), OP_AVG, 3, THIRD).tolist() == [0x3f47, 0x3f9c]
    assert rne(mul(wide(rne(result(wide(_b(0x4130)), OP_AVG, 3, 1.0))), THIRD)).tolist() == [0x3f9d]
    # SUM with b = 1 and AVG at P = 1: the bytes
    assert bh.unpack(_b(0x7f81, 0x8000), OP_SUM, 3, 1.0).tolist() == [0x7f81, 0x8000]
    assert bh.unpack(_b(0x7f81), OP_AVG, 1, 1.0).tolist() == [0x7f81]
    # the statistic is of the stored values: 3 stored as bf16 0x4040 -> 9; 1/3 stored as 0x3eab = 0.333984375
    assert bh.sumsq(_b(0x4040, 0x3f80)) == 10.0
    assert bh.sumsq(_b(0x3eab)) == 0.333984375 ** 2
    assert np.isinf(bh.sumsq(_b(0x7f80, 0x3f80))) and np.isnan(bh.sumsq(_b(0x7fc0))) and bh.sumsq(_b()) == 0.0


def test_b_one_is_the_avg_op():
    """With b == 1 the contract's bits are the AVG op's (torch CPU's bf16 quotient) on every pattern."""
    for P in (2, 3, 5, 7):
        assert differing(bh.unpack(ALL_BITS, OP_AVG, P, 1.0), quotient(DT_BFLOAT16, ALL_BITS, P)) == 0


def test_wrong_engines_are_rejected_by_the_chosen_inputs():
    v = wide(ALL_BITS)
    # a rounding to bf16 between the quotient and the factor
    between = {P: differing(bh.unpack(ALL_BITS, OP_AVG, P, THIRD),
                            rne(mul(wide(rne(result(v, OP_AVG, P, 1.0))), THIRD))) for P in (2, 3)}
    assert between == {2: 86, 3: 13584}  # hence P = 3 with b = 1/3 on the GPU
    # a truncating narrow
    with np.errstate(all='ignore'):
        trunc = (mul(v, THIRD).view(np.uint32) >> 16).astype(np.uint16)
    assert differing(bh.pack(ALL_BITS, THIRD), trunc) == 21926
    # the factor ahead of the quotient: only b = 3 shows it, at the overflow / subnormal edges
    ahead = {}
    for b in bh.FACTORS[1:]:
        with np.errstate(all='ignore'):
            wrong = rne((mul(v, b) / np.float32(3)).astype(np.float32))
        ahead[float(b)] = differing(bh.unpack(ALL_BITS, OP_AVG, 3, b), wrong)
    assert ahead[3.0] == 426 and all(n == 0 for b, n in ahead.items() if b != 3.0), ahead
    # the statistic of the unrounded chain is another number than that of the stored values
    fin = ALL_BITS[np.isfinite(v)]
    stored = bh.unpack(fin, OP_AVG, 3, THIRD)
    assert bh.sumsq(stored) != mirror(result(wide(fin), OP_AVG, 3, THIRD), True)
    assert np.isfinite(bh.sumsq(stored))
    # a value that only overflows in the narrowing: the unrounded chain is finite, what is stored is inf
    edge = _b(0x7f7f)  # * 3 / 3 in fp32 stays finite, * 3 alone does not
    assert np.isinf(bh.sumsq(bh.unpack(edge, OP_SUM, 3, THREE)))
    big = np.array([3.4e38], np.float32)  # finite in fp32, above the rounding boundary 3.3961e38 of the largest bf16 value
    assert np.isfinite(mirror(big, True)) and np.isinf(bh.sumsq(rne(big)))
    # NOT observable through a bf16 store: a reciprocal multiply instead of the quotient (no test claims it)
    for P in (2, 3, 5, 7):
        with np.errstate(all='ignore'):
            rec = rne((v * (np.float32(1) / np.float32(P))).astype(np.float32))
        assert differing(bh.unpack(ALL_BITS, OP_AVG, P, 1.0), rec) == 0


class _FakeCuda:
    """What the checks look at of a dense, contiguous device tensor: nothing is dereferenced."""
    is_sparse, is_cuda = False, True

    def __init__(self, dtype):
        self.dtype = dtype
        self.device = torch.device('cpu')

    def is_contiguous(self):
        return True


def test_python_validation():
    from ddl.torch import cpp_backend as cb
    from ddl.torch import tensor_communicate as tc
    for check in (tc._check_sumsq, tc._check_scale):
        check([_FakeCuda(torch.bfloat16), _FakeCuda(torch.float32)], cb.OP_AVG, 'x')
        for dt in (torch.float16, torch.float64, torch.int32):
            with pytest.raises(ValueError, match='float32'):
                check([_FakeCuda(dt)], cb.OP_SUM, 'x')
        with pytest.raises(ValueError):
            check([_FakeCuda(torch.bfloat16)], cb.OP_MAX, 'x')
        with pytest.raises(ValueError):
            check([torch.zeros(3, dtype=torch.bfloat16)], cb.OP_SUM, 'x')  # host memory


def test_wrapper_hands_bf16_gradients_to_the_engine():
    from ddl.torch.parallelism.data.distributed_optimizer import data_parallelism_distributed_optimizer_wrapper
    base = torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))], lr=0.1)
    opt = data_parallelism_distributed_optimizer_wrapper(base, gradient_predivide_factor=2)
    opt.loss_scale = 8.0
    for dt in (torch.bfloat16, torch.float32):
        assert opt._engine_sumsq(_FakeCuda(dt))
        assert opt._engine_factors(_FakeCuda(dt)) == (0.5, 0.25)
    assert not opt._engine_sumsq(_FakeCuda(torch.float16))
    assert opt._engine_factors(_FakeCuda(torch.float16)) == (1.0, 1.0)
    assert opt._engine_factors(torch.zeros(3, dtype=torch.bfloat16)) == (1.0, 1.0)  # a CPU gradient
