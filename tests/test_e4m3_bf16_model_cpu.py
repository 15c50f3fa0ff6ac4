"""The e4m3 wire over bfloat16 tensors: hand-worked values of the model in _e4m3_bf16_helpers.py, and the Python
surface's decision which tensors a kind compresses. No GPU."""
import types

import numpy as np
import pytest
import torch

import _e4m3_bf16_helpers as h
import _e4m3_helpers as q8

THIRD = float(np.float32(1) / np.float32(3))


def _granule(codes, scale):
    w = np.zeros(256, np.uint8)
    w[:len(codes)] = codes
    w[252:] = np.array([scale], np.float32).view(np.uint8)
    return w


def test_smallest_scale_is_where_narrowing_a_code_is_inexact():
    """At s = 2**-126 the codes 1, 2, 3 decode to 2**-135, 2**-134 and 3 * 2**-135: below bf16's smallest subnormal
    2**-133, they store as 0, 0 (a tie, to even) and 2**-133. From s = 2**-124 on the smallest code is 2**-133 and a
    code times its scale has at most 4 significant bits: narrowing it is exact."""
    w = _granule([1, 2, 3], 2.0 ** -126)
    assert q8.dequantize(w)[:3].tolist() == [2.0 ** -135, 2.0 ** -134, 3 * 2.0 ** -135]
    assert h.unpack(w, 3).tolist() == [0x0000, 0x0000, 0x0001]
    for s in (2.0 ** -124, 1.0, 2.0 ** 120):
        y = q8.dequantize(_granule(np.arange(252, dtype=np.uint8), s))
        keep = np.isfinite(y)
        assert np.array_equal(h.wide(h.rne(y))[keep], y[keep])


def test_one_rounding_at_the_end():
    """AVG at P = 3 with a postscale of 1/3 on the code 0x3b = 1.375 under s = 1: the fp32 quotient times the fp32
    third narrows to 0x3e1c; narrowing the quotient first gives 0x3e1d."""
    assert h.unpack(_granule([0x3b], 1.0), 1, q8.OP_AVG, 3, THIRD).tolist() == [0x3e1c]
    between = h.wide(h.rne((np.float32(1.375) / np.float32(3)).reshape(1)))
    assert h.rne((between * np.float32(THIRD)).astype(np.float32)).tolist() == [0x3e1d]


@pytest.mark.parametrize('kind,dtype,want', [('fp8', torch.float32, True), ('fp8', torch.bfloat16, False),
                                              ('fp8_all', torch.float32, True), ('fp8_all', torch.bfloat16, True),
                                              ('fp8_all', torch.float16, False), ('fp8_feedback', torch.bfloat16, False)])
def test_which_tensors_a_kind_compresses(kind, dtype, want):
    from ddl.torch import cpp_backend as cb
    from ddl.torch.compression import Compression, wire_flag
    from ddl.torch.tensor_communicate import _compressible
    comm, c = types.SimpleNamespace(size=2), getattr(Compression, kind)
    assert _compressible(torch.zeros(8, dtype=dtype), comm, c, cb.MEMORY_DEVICE) is want
    assert not _compressible(torch.zeros(8, dtype=dtype), comm, c, cb.MEMORY_HOST)
    assert wire_flag(Compression.fp8_all) == wire_flag(Compression.fp8) == cb.WIRE_E4M3
