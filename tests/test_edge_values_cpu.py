"""The every-pattern input sets of tests/_edge_helpers.py, checked on the CPU before the GPU tests
(tests/test_edge_values_gpu.py) rely on them:

  * the oracle agrees with numpy (fp16) / torch CPU (bf16) on the whole sets;
  * the sets hold what they are for (subnormal results, overflow to inf from finite inputs, NaNs that
    do not swamp the set, exact ties rounded both ways): floors are asserted, the counts printed
    (pytest -s shows them);
  * a subtly wrong kernel would fail: every mutant of the reference is rejected by the comparator on
    at least 1000 elements.
"""
import numpy as np
import pytest

import _edge_helpers as eh
from _avg_helpers import assert_same, is_nan
from _helpers import DT_BFLOAT16, DT_DOUBLE, DT_FLOAT, DT_HALF, NAME
from _wire_helpers import narrow, widen

HALF_IDS = dict(ids=lambda d: NAME[d])
FOLD_NB = [1, 2, 7, 15]
FLOOR = 1000          # elements of every class, and witnesses against every mutant
MAX_NAN_SHARE = 0.30


def _rejected(dt, got, want, what):
    """assert_same refuses `got`; returns how many elements it has to refuse."""
    with pytest.raises(AssertionError):
        assert_same(dt, got, want, what)
    return eh.count_diffs(dt, got, want)


# ---- shapes of the sets ----------------------------------------------------------------------------
@pytest.mark.parametrize('dt', eh.HALF_TYPES, **HALF_IDS)
def test_pair_set_layout(dt):
    a, b = eh.pair_bits(dt)
    assert a.size == b.size == eh.N_PAIRS == 1_703_936 and eh.N_GROUPS == 26
    for g in range(eh.N_GROUPS):
        assert np.array_equal(a[g << 16:(g + 1) << 16], eh.patterns())
    for g, v in enumerate(eh.FIXED[dt]):
        assert (b[g << 16:(g + 1) << 16] == v).all()
    pa, pb = eh.pair_set(dt, tail=True)
    assert pa.size == pb.size == eh.N_PAIRS + 7 and pa.size % 8 == 7


def test_derived_partners_by_hand():
    """a, -a, one pattern further from zero with the other sign, ±half an ulp: values worked by hand."""
    h = np.array([0x3c00, 0xbc00, 0x7bff, 0x7c00, 0xfe01, 0x0000, 0x03ff, 0x0400, 0x0800, 0x2c00, 0x3000], np.uint16)
    same, neg, step, hp, hn = eh.derived_partners(DT_HALF, h)
    assert same.tolist() == h.tolist() and neg.tolist() == (h ^ 0x8000).tolist()
    assert step.tolist()[:6] == [0xbc01, 0x3c01, 0xfc00, 0xfc00, 0x7e01, 0x8001]
    # half an ulp of 1.0 is 2^-11 (field 4); of 2^-14 (field 1) and below: not representable; of 2^-13
    # (field 2) it is 2^-24, the smallest subnormal; of 2^-4 (field 11) 2^-15 = 0x0200; field 12: 2^-14
    assert hp.tolist() == [0x1000, 0x9000, 0x4c00, 0x5000, 0xd000, 0, 0, 0, 0x0001, 0x0200, 0x0400]
    assert (hn ^ hp).tolist() == [0x8000] * h.size
    b = np.array([0x3f80, 0x0080, 0x0100, 0x0400, 0x0480, 0xff7f], np.uint16)
    _, _, step, hp, _ = eh.derived_partners(DT_BFLOAT16, b)
    # bf16: 1.0 (field 127) -> 2^-8 (field 119); field 1: none; field 2: 2^-133; field 8: 2^-127 = 0x0040
    assert hp.tolist() == [0x3b80, 0, 0x0001, 0x0040, 0x0080, 0xfb00] and step[5] == 0x7f80
    # the value: a + half an ulp is an exact tie for normals (checked in fp64 for fp16)
    one = widen(DT_HALF, eh.storage(DT_HALF, h[:1])).astype(np.float64)
    half = widen(DT_HALF, eh.storage(DT_HALF, eh.derived_partners(DT_HALF, h[:1])[3])).astype(np.float64)
    assert one[0] + half[0] == 1.0 + 2.0 ** -11


@pytest.mark.parametrize('dt', eh.HALF_TYPES, **HALF_IDS)
def test_fold_set_layout(dt):
    xs = eh._fold_bits(dt, 15)
    a, b = eh.pair_bits(dt)
    assert len(xs) == 16 and all(x.size == eh.N_PAIRS for x in xs)
    assert xs[0] is a and xs[1] is b
    for g in range(eh.N_GROUPS):
        h = (g + 5) % eh.N_GROUPS
        assert np.array_equal(xs[2][g << 16:(g + 1) << 16], b[h << 16:(h + 1) << 16])
    q = eh.fold_partners(dt)
    assert len(q) == 10 and q[0] == 0 and all(v < eh.INF[dt] for v in q)
    assert eh.is_subnormal(dt, np.array([q[2], q[6]], np.uint16)).all()  # the unpaired input at nb = 7 and 15
    for i in range(3, 16, 2):
        assert (xs[i] == q[(i - 3) // 2]).all()
        if i + 1 < 16:
            assert (xs[i + 1] == xs[i] | 0x8000).all()
    assert all(np.array_equal(u, v) for u, v in zip(eh._fold_bits(dt, 7), xs))  # a prefix of the longer set


@pytest.mark.parametrize('dt', eh.HALF_TYPES, **HALF_IDS)
def test_pack_set_layout(dt):
    x = eh.pack_set(dt)                     # asserts inside that every midpoint is exact in fp32
    mid = eh.pack_midpoints(dt)
    n = eh.INF[dt]
    assert x.size == {DT_HALF: 253_966, DT_BFLOAT16: 261_134}[dt]
    per_sign = (x.size - 14) // 2
    assert mid.sum() == 2 * n
    # every finite wire pattern is there as its own value, and converts back to itself
    w = np.concatenate([np.arange(n), 0x8000 + np.arange(n)]).astype(np.uint16)
    vals = np.concatenate([x[:n], x[per_sign:per_sign + n]])
    assert np.array_equal(widen(dt, eh.storage(dt, w)).view(np.uint32), vals.view(np.uint32))
    # a midpoint lies between two wire patterns: it is no wire value, and rounds to the even one
    m = x[mid]
    back = widen(dt, narrow(dt, m))
    assert (back != m).all()
    assert (eh.bits_of(narrow(dt, m)) & 1 == 0).all()
    assert np.isnan(x[-10:]).all() and np.isinf(x[-14:-12]).all()
    assert np.array_equal(x[-10:].view(np.uint32), eh.PACK_NANS)


@pytest.mark.parametrize('dt', eh.FLOAT_TYPES, **HALF_IDS)
def test_edge_table_layout(dt):
    E = eh.edge_values(dt)
    f = np.finfo(E.dtype)
    assert 36 <= E.size <= 44
    for v in (0.0, f.smallest_subnormal, f.tiny, f.max, f.max / 2, -f.max / 2, np.nextafter(f.max, E.dtype.type(0)), 1.0,
              1.0 + f.eps, -1.0, 2.0 ** -60, np.inf, -np.inf):
        assert (E == E.dtype.type(v)).any(), v
    assert np.isnan(E).any() and np.signbit(E[E == 0]).any()
    a, b = eh.edge_table(dt)
    assert a.size == E.size ** 2 + eh.TABLE_TAIL and a.size % (16 // E.itemsize) != 0


# ---- the oracle against numpy / torch on the whole sets --------------------------------------------
@pytest.mark.parametrize('dt', eh.HALF_TYPES, **HALF_IDS)
def test_oracle_sum2_is_the_cpu_cast_of_the_fp32_sum(oracle, dt):
    a, b = eh.pair_set(dt, tail=True)
    got, want = oracle.sum2(dt, a, b), eh.np_fold(dt, [a, b])
    assert np.array_equal(is_nan(dt, got), is_nan(dt, want))
    assert eh.count_diffs(dt, got, want) == 0
    assert_same(dt, got, want, f'oracle sum2 {NAME[dt]}')


@pytest.mark.parametrize('nb', FOLD_NB)
@pytest.mark.parametrize('dt', eh.HALF_TYPES, **HALF_IDS)
def test_oracle_fold_is_the_cpu_cast_of_the_fp32_fold(oracle, dt, nb):
    xs = eh.fold_set(dt, nb)
    assert_same(dt, oracle.fold(dt, xs), eh.np_fold(dt, xs), f'oracle fold {NAME[dt]} nb={nb}')
    assert_same(dt, oracle.allreduce_seq(dt, xs), eh.np_fold(dt, xs, each_add=True), f'oracle seq {NAME[dt]} nb={nb}')
    for total in (4096, 0):  # fp16 / bf16 keep the left fold whatever the order
        assert oracle.fold_ref_order(dt, xs, total).tobytes() == oracle.fold(dt, xs).tobytes()


@pytest.mark.parametrize('dt', eh.HALF_TYPES, **HALF_IDS)
def test_oracle_casts_are_the_cpu_casts(oracle, dt):
    """ddlo_float_to_half / ddlo_float_to_bf16, element by element over the pack set."""
    import ctypes
    x = eh.pack_set(dt)
    fn = oracle.lib.ddlo_float_to_half if dt == DT_HALF else oracle.lib.ddlo_float_to_bf16
    # c_float arguments that share the input's bytes: a Python float in between would quieten a
    # signalling NaN before the oracle sees it
    raw = bytearray(x.tobytes())
    got = np.fromiter((fn(ctypes.c_float.from_buffer(raw, o)) for o in range(0, len(raw), 4)), dtype=np.uint16,
                      count=x.size)
    want = narrow(dt, x)
    assert np.array_equal(is_nan(dt, eh.storage(dt, got)), is_nan(dt, want))
    assert eh.count_diffs(dt, eh.storage(dt, got), want) == 0
    assert np.array_equal(is_nan(dt, want), np.isnan(x))


@pytest.mark.parametrize('dt', eh.FLOAT_TYPES, **HALF_IDS)
def test_oracle_fp32_fp64_is_numpy_plus(oracle, dt):
    a, b = eh.edge_table(dt)
    c = b[::-1].copy()
    assert_same(dt, oracle.sum2(dt, a, b), eh.np_add([a, b]), NAME[dt])
    assert_same(dt, oracle.fold(dt, [a, b, c]), eh.np_add([a, b, c]), NAME[dt])
    assert_same(dt, oracle.fold_ref_order(dt, [a, b, c], 4096), eh.np_add([a, b, c]), NAME[dt])
    with np.errstate(all='ignore'):
        s = a + b
    f = np.finfo(a.dtype)
    fin = np.isfinite(a) & np.isfinite(b)
    sub = (s != 0) & (np.abs(s) < f.tiny)
    print(f'{NAME[dt]} table: {a.size} pairs, {int(sub.sum())} subnormal sums, {int((np.isinf(s) & fin).sum())} '
          f'finite->inf, {int(np.isnan(s).sum())} NaN, {int((np.isnan(s) & ~np.isnan(a) & ~np.isnan(b)).sum())} inf-inf')
    assert sub.sum() >= 50 and (np.isinf(s) & fin).sum() >= 10 and (np.isnan(s) & ~np.isnan(a) & ~np.isnan(b)).sum() >= 2


# ---- the sets contain what they are for --------------------------------------------------------------
def _check_classes(what, c):
    print(f'{what}: subnormal {c["subnormal"]}, finite->inf {c["finite_to_inf"]}, NaN {c["nan"]} '
          f'(share {c["nan_share"]:.3f})')
    assert c['subnormal'] >= FLOOR and c['finite_to_inf'] >= FLOOR and c['nan'] >= FLOOR, (what, c)
    assert c['nan_share'] <= MAX_NAN_SHARE, (what, c)


@pytest.mark.parametrize('dt', eh.HALF_TYPES, **HALF_IDS)
def test_pair_set_holds_every_class(oracle, dt):
    a, b = eh.pair_set(dt)
    _check_classes(f'sum2 {NAME[dt]}', eh.classes(dt, [a, b], oracle.sum2(dt, a, b)))
    if dt == DT_BFLOAT16:
        ties, down = eh.bf16_ties([a, b])
        print(f'sum2 bfloat16: {ties} exact ties, {down} to the even pattern below, {ties - down} above')
        assert down >= FLOOR and ties - down >= FLOOR


@pytest.mark.parametrize('nb', FOLD_NB)
@pytest.mark.parametrize('dt', eh.HALF_TYPES, **HALF_IDS)
def test_fold_set_holds_every_class(oracle, dt, nb):
    xs = eh.fold_set(dt, nb)
    _check_classes(f'fold {NAME[dt]} nb={nb}', eh.classes(dt, xs, oracle.fold(dt, xs)))


@pytest.mark.parametrize('dt', eh.HALF_TYPES, **HALF_IDS)
def test_pack_set_holds_every_class(dt):
    x = eh.pack_set(dt)
    w = narrow(dt, x)
    sub, inf = eh.is_subnormal(dt, w), eh.is_inf(dt, w) & np.isfinite(x)
    print(f'pack {NAME[dt]}: {x.size} elements, {int(eh.pack_midpoints(dt).sum())} exact ties, {int(sub.sum())} '
          f'subnormal results, {int(inf.sum())} finite->inf, {int(np.isnan(x).sum())} NaN')
    n_sub = 2 * (eh.MIN_NORMAL[dt] - 1)
    assert sub.sum() >= 3 * n_sub          # its value and the nearer neighbour of the midpoint on either side
    assert inf.sum() >= 6                  # per sign: the last midpoint, its upper neighbour, the largest fp32
    assert np.isnan(x).sum() == 10


# ---- a wrong kernel would fail -----------------------------------------------------------------------
def _mutants(dt, xs):
    """(name, what the mutant computes for the inputs xs) for the 16-bit reduce / fold."""
    ref = eh.np_fold(dt, xs)
    out = [('results flushed to zero', eh.flush_results(dt, ref)),
           ('subnormal inputs read as zero', eh.np_fold(dt, [eh.flush_inputs(dt, x) for x in xs])),
           ('overflow saturated to max', eh.saturate(dt, xs, ref)),
           ('ties rounded away from zero', eh.np_fold(dt, xs, narrow_fn=lambda s: eh.narrow_ties_away(dt, s)))]
    if dt == DT_BFLOAT16:
        out.append(('rounded by truncation', eh.np_fold(dt, xs, narrow_fn=eh.narrow_truncate_bf16)))
    return out


@pytest.mark.parametrize('dt', eh.HALF_TYPES, **HALF_IDS)
def test_sum2_mutants_are_rejected(oracle, dt):
    a, b = eh.pair_set(dt)
    want = oracle.sum2(dt, a, b)
    for name, got in _mutants(dt, [a, b]):
        k = _rejected(dt, got, want, name)
        print(f'sum2 {NAME[dt]}, {name}: {k} witnesses')
        assert k >= FLOOR, (name, k)


@pytest.mark.parametrize('nb', FOLD_NB)
@pytest.mark.parametrize('dt', eh.HALF_TYPES, **HALF_IDS)
def test_fold_mutants_are_rejected(oracle, dt, nb):
    xs = eh.fold_set(dt, nb)
    want = oracle.fold(dt, xs)
    todo = _mutants(dt, xs)
    if nb >= 2:
        todo.append(('rounded after every add', oracle.allreduce_seq(dt, xs)))
    for name, got in todo:
        k = _rejected(dt, got, want, name)
        print(f'fold {NAME[dt]} nb={nb}, {name}: {k} witnesses')
        assert k >= FLOOR, (name, k)


@pytest.mark.parametrize('dt', eh.HALF_TYPES, **HALF_IDS)
def test_pack_mutants_are_rejected(dt):
    x = eh.pack_set(dt)
    want = narrow(dt, x)
    n_ties = int(eh.pack_midpoints(dt).sum())
    n_sub = 2 * (eh.MIN_NORMAL[dt] - 1)
    # ties away: wrong on every tie whose even neighbour is the lower one (every other pattern); flushed:
    # on everything that rounds to a subnormal; truncation: on every upper neighbour of a midpoint and on
    # every tie that rounds up
    todo = [('ties rounded away from zero', eh.storage(dt, eh.narrow_ties_away(dt, x)), n_ties // 2 - 2),
            ('results flushed to zero', eh.flush_results(dt, want), 3 * n_sub)]
    if dt == DT_BFLOAT16:
        todo.append(('rounded by truncation', eh.narrow_truncate_bf16(x), n_ties))
    for name, got, floor in todo:
        k = _rejected(dt, got, want, name)
        print(f'pack {NAME[dt]}, {name}: {k} witnesses (floor {floor})')
        assert k >= floor >= 750, (name, k)


def test_pack_bf16_rounding_without_a_nan_test_is_rejected():
    """(u + 0x7fff + lsb) >> 16 on a NaN whose payload lies below the kept bits carries into inf (or
    past it, into -0): 5 of the 10 NaNs of the set stop being NaNs, and nothing else differs."""
    x = eh.pack_set(DT_BFLOAT16)
    want, got = narrow(DT_BFLOAT16, x), eh.narrow_bf16_no_nan_test(x)
    assert _rejected(DT_BFLOAT16, got, want, 'no NaN test') == 5
    lost = is_nan(DT_BFLOAT16, want) & ~is_nan(DT_BFLOAT16, got)
    assert lost.sum() == 5 and np.array_equal(x.view(np.uint32)[lost],
                                              [0x7f800001, 0x7f801fff, 0x7f802000, 0xff800001, 0x7fffffff])


def test_float_table_mutants_are_rejected():
    """fp32 / fp64: flushing subnormal sums, or reading subnormal inputs as zero, shows on the table."""
    for dt in (DT_FLOAT, DT_DOUBLE):
        a, b = eh.edge_table(dt)
        want = eh.np_add([a, b])
        f = np.finfo(a.dtype)
        flushed = np.where((want != 0) & (np.abs(want) < f.tiny), np.copysign(0, want), want).astype(a.dtype)
        za, zb = (np.where((v != 0) & (np.abs(v) < f.tiny), np.copysign(0, v), v).astype(a.dtype) for v in (a, b))
        for name, got in (('results flushed', flushed), ('inputs flushed', eh.np_add([za, zb]))):
            k = _rejected(dt, got, want, name)
            print(f'{NAME[dt]} table, {name}: {k} witnesses')
            assert k >= 50, (name, k)
