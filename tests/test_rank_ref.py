"""
CPU tests of the rank reference itself (tests/rank_ref.py): the loops against independent routes -- argsort ranks on tie-free
data, S on monotone columns, an all-equal column, the sum invariant of the statistics 1 to 5, tie3 against an explicit grouping,
the swap of a and b -- the row-vector and small-alphabet references against the loops, and scipy where it is installed.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rank_ref as R                                                      # noqa: E402


def test_argsort_ranks_on_tie_free_data():
    rng = np.random.default_rng(1)
    a = rng.permutation(40 * 3).reshape(40, 3).astype(np.float32)
    ra, rb, st = R.reference(a)
    assert rb is None
    want = np.argsort(np.argsort(a, axis=0), axis=0) + 1
    assert np.array_equal(ra, want.astype(np.float32)) and not st[3:].any()


def test_monotone_and_all_equal_columns():
    T = 23
    t = np.arange(T, dtype=np.float32)
    a = np.stack([t, -t, np.full(T, 4.0, np.float32)], axis=1)
    st = R.reference(a)[2]
    n2 = T * (T - 1) // 2
    assert st[1].tolist() == [n2, 0, 0] and st[2].tolist() == [0, n2, 0] and st[3].tolist() == [0, 0, n2]
    assert st[6].tolist() == [0, 0, T * (T - 1) * (2 * T + 5)] and not st[[4, 5, 7]].any()
    ra, rb, sp = R.reference(a, a.copy())
    assert sp[5].tolist() == [0, 0, n2] and sp[1].tolist() == [n2, n2, 0] and not sp[[2, 3, 4]].any()
    assert np.array_equal(ra, rb) and (ra[:, 2] == np.float32((T + 1) / 2)).all()


@pytest.mark.parametrize('form', [R.TREND, R.PAIR, R.INDEX])
@pytest.mark.parametrize('values,holes', [('ties', 'scattered'), ('special', 'b only'), ('noise', 'column')])
def test_invariants_and_the_vector_reference(form, values, holes):
    rng = np.random.default_rng(7 + form)
    a, b = R.make(rng, 29, 6, form, values, holes)
    for mode in R.MODES:
        ra, rb, st = R.reference(a, b, mode)
        va, vb, vs = R.reference_rows(a, b, mode)
        assert np.array_equal(R.bits(ra), R.bits(va)) and np.array_equal(st, vs)
        assert (rb is None) == (vb is None) and (rb is None or np.array_equal(R.bits(rb), R.bits(vb)))
    ra, rb, st = R.reference(a, b)
    n = st[0]
    assert np.array_equal(st[1:6].sum(axis=0), n * (n - 1) // 2)
    bb = None if b is None else (np.broadcast_to(b[:, None], a.shape) if b.ndim == 1 else b)
    for e in range(a.shape[1]):
        ok = ~np.isnan(a[:, e]) if bb is None else ~np.isnan(a[:, e]) & ~np.isnan(bb[:, e])
        assert st[6, e] == R.tie3_by_groups(a[ok, e])
        assert st[7, e] == (0 if bb is None else R.tie3_by_groups(bb[ok, e]))
    if form == R.TREND:
        assert not st[[4, 5, 7]].any()
    if form == R.PAIR:
        sa, sb, ss = R.reference(b, a)
        assert np.array_equal(ss[[0, 1, 2, 4, 3, 5, 7, 6]], st) and np.array_equal(R.bits(sa), R.bits(rb))
    # propagate: a column with a hole is -1 but for n_valid, and every rank NaN
    pa, pb, ps = R.reference(a, b, R.PROPAGATE)
    holed = n < a.shape[0]
    assert (ps[1:, holed] == -1).all() and np.array_equal(ps[:, ~holed], st[:, ~holed]) and np.array_equal(ps[0], n)
    assert np.isnan(pa[:, holed]).all() and np.array_equal(R.bits(pa[:, ~holed]), R.bits(ra[:, ~holed]))
    assert (R.bits(pa)[np.isnan(pa)] == R.QNAN).all()


def test_signed_zeros_and_infinities_are_values():
    a = np.array([[0.0], [-0.0], [np.inf], [np.inf], [-np.inf], [np.nan]], dtype=np.float32)
    ra, _, st = R.reference(a)
    assert ra[:5, 0].tolist() == [2.5, 2.5, 4.5, 4.5, 1.0] and np.isnan(ra[5, 0])
    assert st[:, 0].tolist() == [5, 4, 4, 2, 0, 0, 2 * 2 * 9, 0]


def test_the_small_alphabet_count():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 3, (50, 4)).astype(np.float32)
    assert np.array_equal(R.small_alphabet_stats(a), R.reference(a)[2])


def test_scipy_agrees_where_it_is_installed():
    try:
        import scipy.stats as ss
    except ImportError:                                                 # an extra cross-check, nothing depends on it
        return
    rng = np.random.default_rng(5)
    a, b = R.make(rng, 31, 4, R.PAIR, 'ties', 'scattered')
    ra, rb, st = R.reference(a, b)
    for e in range(4):
        ok = ~np.isnan(a[:, e]) & ~np.isnan(b[:, e])
        assert np.array_equal(ra[ok, e], ss.rankdata(a[ok, e]).astype(np.float32))
        C, D, Ta, Tb = (int(st[k, e]) for k in (1, 2, 3, 4))
        tau = (C - D) / np.sqrt(float((C + D + Ta) * (C + D + Tb)))
        assert abs(tau - ss.kendalltau(a[ok, e], b[ok, e]).statistic) < 1e-12
