"""The MIN / MAX reference model (tests/_minmax_helpers.py) against a slow per-element Python model
on the float edge set, as all ordered pairs, for all four float types. The slow model decodes every
pattern to an exact Python number (fractions, no floating-point compare) and orders zeros by sign."""
from fractions import Fraction

import numpy as np
import pytest

from _helpers import DT_BFLOAT16, DT_DOUBLE, DT_FLOAT, DT_HALF, DT_INT32, DT_INT64, DT_UINT64, NAME, NP
from _minmax_helpers import (FLOAT_DTYPES, OP_MAX, OP_MIN, OPS, edge_bits, edge_pairs, float_bits, is_nan, model,
                             nan_bits)

LAYOUT = {DT_HALF: (16, 10, 15), DT_BFLOAT16: (16, 7, 127), DT_FLOAT: (32, 23, 127), DT_DOUBLE: (64, 52, 1023)}


def decode(dt, bits):
    """('nan',) or (exact value, rank of the sign for zeros): a totally ordered Python key."""
    w, m, bias = LAYOUT[dt]
    bits = int(bits)
    neg = bits >> (w - 1)
    e, frac = (bits >> m) & ((1 << (w - 1 - m)) - 1), bits & ((1 << m) - 1)
    emax = (1 << (w - 1 - m)) - 1
    if e == emax and frac:
        return None
    if e == emax:
        v = Fraction(10) ** 400  # beyond every finite value
    elif e == 0:
        v = Fraction(frac) * Fraction(2) ** (1 - bias - m)
    else:
        v = Fraction(frac + (1 << m)) * Fraction(2) ** (e - bias - m)
    return (-v if neg else v, 0 if neg else 1)  # -0 < +0


def slow(dt, op, a_bits, b_bits):
    out = []
    for a, b in zip(a_bits.tolist(), b_bits.tolist()):
        ka, kb = decode(dt, a), decode(dt, b)
        if ka is None or kb is None:
            out.append(None)
        elif op == OP_MAX:
            out.append(a if ka >= kb else b)
        else:
            out.append(a if ka <= kb else b)
    return out


@pytest.mark.parametrize('op', OPS)
@pytest.mark.parametrize('dt', FLOAT_DTYPES, ids=lambda d: NAME[d])
def test_model_matches_the_slow_model_on_all_edge_pairs(dt, op):
    a, b = edge_pairs(dt)
    got = model(dt, op, [a, b])
    want = slow(dt, op, float_bits(dt, a), float_bits(dt, b))
    gb = float_bits(dt, got)
    assert len(want) == edge_bits(dt).size ** 2 == gb.size
    nans = 0
    for i, w in enumerate(want):
        if w is None:
            assert nan_bits(dt, gb[i:i + 1])[0], i
            nans += 1
        else:
            assert int(gb[i]) == w, (i, hex(int(gb[i])), hex(w))
    assert nans > 0 and nans < len(want)
    # the NaN the model returns is quiet, and is_nan (the comparison rule's test) sees it
    assert is_nan(dt, got).sum() == nans


def test_edge_set_holds_what_the_contract_names():
    for dt in FLOAT_DTYPES:
        e = edge_bits(dt)
        assert len(set(e.tolist())) == e.size
        n = nan_bits(dt, e)
        assert n.sum() == 5 and (~n).sum() == 18
        vals = [decode(dt, x) for x in e[~n]]
        assert (Fraction(0), 0) in vals and (Fraction(0), 1) in vals and (Fraction(1), 1) in vals


def test_signed_zero_nan_and_integer_rules():
    f = np.float32
    z = model(DT_FLOAT, OP_MAX, [np.array([-0.0, 0.0], f), np.array([0.0, -0.0], f)])
    assert not np.signbit(z).any()
    z = model(DT_FLOAT, OP_MIN, [np.array([-0.0, 0.0], f), np.array([0.0, -0.0], f)])
    assert np.signbit(z).all()
    for op in OPS:  # a NaN never hides, whatever its position
        for pos in range(3):
            xs = [np.array([1.0], f), np.array([2.0], f), np.array([3.0], f)]
            xs[pos] = np.array([np.nan], f)
            assert np.isnan(model(DT_FLOAT, op, xs)).all()
    s = np.array([-5, 7, np.iinfo(np.int64).min], np.int64)
    t = np.array([3, -7, np.iinfo(np.int64).max], np.int64)
    assert model(DT_INT64, OP_MAX, [s, t]).tolist() == [3, 7, np.iinfo(np.int64).max]
    assert model(DT_INT32, OP_MIN, [s.astype(np.int32)[:2], t.astype(np.int32)[:2]]).tolist() == [-5, -7]
    u = s.view(np.uint64)
    assert model(DT_UINT64, OP_MAX, [u, t.view(np.uint64)]).tolist() == [int(u[0]), int(t.view(np.uint64)[1]), int(u[2])]
    assert model(DT_UINT64, OP_MAX, [u]).dtype == NP[DT_UINT64]


def test_model_is_associative_and_commutative():
    rng = np.random.default_rng(5)
    for dt in FLOAT_DTYPES:
        e = edge_bits(dt)
        xs = [rng.choice(e, 4000).view(NP[dt]) for _ in range(5)]
        for op in OPS:
            want = float_bits(dt, model(dt, op, xs))
            nan = nan_bits(dt, want)
            for perm in ([4, 3, 2, 1, 0], [2, 0, 4, 1, 3]):
                ys = [xs[i] for i in perm]
                step = model(dt, op, [model(dt, op, ys[:2]), model(dt, op, ys[2:])])
                g = float_bits(dt, step)
                assert np.array_equal(nan_bits(dt, g), nan) and np.array_equal(g[~nan], want[~nan])
