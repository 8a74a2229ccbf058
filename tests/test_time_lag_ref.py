"""
CPU tests of tests/time_lag_ref.py: the numpy restatement of dlwpcs_time_lag that the device test compares bits against, its
case tables and its error bound.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time_lag_ref as R         # noqa: E402


def _small(seed, T=37, E=5, pattern='one percent'):
    rng = np.random.default_rng(seed)
    a, b = R.make_series(rng, T, E, pattern)
    a[3, 1] = np.nan
    b[7, 2] = np.nan
    return a, b


@pytest.mark.parametrize('form', ['auto', 'pair', 'index'])
@pytest.mark.parametrize('centred', [False, True])
def test_reference_against_a_naive_double_loop(form, centred):
    """the vectorised reference, its plain-loop twin and a float64 evaluation with numpy's own sums"""
    a, b = _small(1)
    b = {'auto': None, 'pair': b, 'index': b[:, 0].copy()}[form]
    ca = R.centre(a) if centred else None
    cb = None if not centred or b is None else R.centre(b)
    lags = [-40, -36, -3, 0, 1, 2, 36, 37, 50]
    for mode, mc in R.MODES:
        got, n = R.reference(a, b, lags, ca, cb, mode, mc)
        loops, nl = R.reference_loops(a, b, lags, ca, cb, mode, mc)
        assert np.array_equal(R.bits(got), R.bits(loops)) and np.array_equal(n, nl)
        want, nw = R.naive(a, b, lags, ca, cb, mode, mc)
        assert np.array_equal(n, nw) and np.array_equal(np.isnan(got), np.isnan(want))
        fin = ~np.isnan(want)
        assert np.abs(got[fin] - want[fin]).max() <= 3e-6 * np.abs(want[fin]).max()
        assert (n[[0, 7, 8]] == 0).all() and np.isnan(got[[0, 7, 8]]).all()         # |l| >= T: no pairs
        assert (R.bits(got)[np.isnan(got)] == R.QNAN).all()


def test_prototype_case_of_the_issue():
    """T = 1025 with 1 % NaN, a whole-NaN column, NaN at rows 511 and 512; lags up to and beyond the series"""
    rng = np.random.default_rng(2)
    a, _ = R.make_series(rng, 1025, 6, 'one percent')
    a[:, 2] = np.nan
    a[511:513, 4] = np.nan
    ca = R.centre(a)
    lags = [-600, -1, 0, 1, 33, 600, 1024, 1025, 2000]
    got, n = R.reference(a, None, lags, ca)
    want, nw = R.naive(a, None, lags, ca)
    assert np.array_equal(n, nw) and (n[7:] == 0).all() and np.isnan(got[7:]).all() and np.isnan(got[:, 2]).all() and (n[:, 2] == 0).all()
    fin = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), ~fin)
    var = want[2][~np.isnan(want[2])].max()
    assert np.abs(got[fin] - want[fin]).max() <= 3e-6 * var


def test_products_of_float32_are_exact_in_float64():
    """24 x 24 significand bits fit into 53: the product of two float32 in float64 has no rounding, so an fma has the bits of a
    multiply and an add"""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(4000) * 10.0 ** rng.integers(-20, 20, 4000)).astype(np.float32)
    y = (rng.standard_normal(4000) * 10.0 ** rng.integers(-15, 15, 4000)).astype(np.float32)
    x[:4] = np.float32([1 + 2.0 ** -23, 2 - 2.0 ** -23, 3.4e38, 1.2e-38])
    y[:4] = np.float32([1 + 2.0 ** -23, 2 - 2.0 ** -23, 3.4e38, 1.2e-38])
    p = x.astype(np.float64) * y.astype(np.float64)
    for a, b, c in zip(x[:600], y[:600], p[:600]):
        assert Fraction(float(a)) * Fraction(float(b)) == Fraction(float(c))
    m = np.frexp(p)[0] * 2.0 ** 48                      # at most 48 significant bits
    assert np.array_equal(m, np.round(m))


@pytest.mark.parametrize('T', [513, 1025])
def test_the_two_forms_of_the_reference_agree(T):
    """adding a slab sum as soon as it is finished, or keeping them all and adding afterwards: the same additions"""
    rng = np.random.default_rng(T)
    a, b = R.make_series(rng, T, 4, 'slab edge')
    ca, cb = R.centre(a), R.centre(b)
    lags = [-600, -9, 0, 1, 511, 512, 513, T - 1, T]
    one, n1 = R.reference(a, b, lags, ca, cb, split=False)
    two, n2 = R.reference(a, b, lags, ca, cb, split=True)
    assert np.array_equal(R.bits(one), R.bits(two)) and np.array_equal(n1, n2)
    # and the slabs are really there: one sum over all rows rounds differently somewhere
    da, _ = R.deviations(a, ca)
    flat = np.cumsum(da * da, axis=0)[-1] / T
    assert not np.array_equal(R.bits(flat.astype(np.float32)), R.bits(R.reference(a, None, [0], ca)[0][0])) or T <= R.SLAB


def test_slab_of_a_pair_is_the_slab_of_its_a_row():
    """lag 600 at T = 1025: rows 0 .. 424 pair, all in slab 0, although their partners lie in slabs 1 and 2"""
    rng = np.random.default_rng(5)
    a, _ = R.make_series(rng, 1025, 2)
    da, _ = R.deviations(a, None)
    want = np.cumsum(np.concatenate([np.zeros((1, 2)), da[:425] * da[600:]]), axis=0)[-1] / 425
    got, n = R.reference(a, None, [600])
    assert (n == 425).all() and np.array_equal(R.bits(got[0]), R.bits(want.astype(np.float32)))


@pytest.mark.parametrize('T', R.ROWS)
def test_every_lag_set_has_a_lag_with_pairs_and_one_without(T):
    for name, lags in R.lag_sets(T).items():
        assert 1 <= len(lags) <= R.MAX_LAGS
        d = np.diff(lags)
        assert len(lags) == 1 or (d[0] >= 1 and (d == d[0]).all()), name
    pairs = [any(abs(l) < T for l in lags) for lags in R.lag_sets(T).values()]
    none = [any(abs(l) >= T for l in lags) for lags in R.lag_sets(T).values()]
    assert any(pairs) and any(none)
    # per case of the device table: the sets run together, so every case holds both kinds
    assert any(abs(l) < T for lags in R.lag_sets(T).values() for l in lags)
    assert any(abs(l) >= T for lags in R.lag_sets(T).values() for l in lags)
    for w in R.BLOCKS:
        for L in (w - 1, w, w + 1):
            assert L < 1 or '0..%d' % L in R.lag_sets(T)


def test_missing_entries_and_modes():
    a = np.float32([[1.], [np.nan], [3.], [4.], [np.inf]])
    got, n = R.reference(a, None, [0, 1, 2], None, None, R.SKIP, 1)
    assert n[:, 0].tolist() == [4, 2, 2]
    assert np.isinf(got[0, 0]) and got[1, 0] == np.float32((3. * 4. + 4. * np.inf) / 2) and got[2, 0] == np.float32((1. * 3. + 3. * np.inf) / 2)
    got, n = R.reference(a, None, [0, 1], None, None, R.SKIP, 3)
    assert not np.isnan(got[0, 0]) and np.isnan(got[1, 0])
    got, n = R.reference(a, None, [0, 1], None, None, R.PROPAGATE, 1)
    assert np.isnan(got).all() and n[:, 0].tolist() == [4, 2]
    got, n = R.reference(a[2:4], None, [0, 1, -1], None, None, R.PROPAGATE, 1)
    assert got[:, 0].tolist() == [12.5, 12., 12.]
    # inf * 0 of a missing partner is NaN: IEEE decides
    b = np.float32([[np.nan], [1.]])
    got, n = R.reference(np.float32([[np.inf], [2.]]), b, [0])
    assert n[0, 0] == 1 and R.bits(got)[0, 0] == R.QNAN


def test_bound_is_small_on_the_verify_cases_and_holds_for_the_reference():
    """AR(1), phi = 0.8, on an offset of 5500: the bound stays below 1e-5 of the lag-0 variance, and the reference with the float32
    centre lies inside it"""
    rng = np.random.default_rng(8)
    for nan_fraction in (0.0, 0.01):
        a = R.ar1(rng, 600, 16, nan_fraction=nan_fraction)
        b = R.ar1(rng, 600, 16, nan_fraction=nan_fraction)
        for second in (None, b, b[:, 0].copy()):
            lags = list(range(-20, 21))
            exact, lim = R.bound(a, second, lags)
            var = R.bound(a, None, [0])[0][0]
            assert (lim <= 1e-5 * var).all() and (lim > 0).all()
            cb = None if second is None else R.centre(second)
            got, _ = R.reference(a, second, lags, R.centre(a), cb)
            assert (np.abs(got.astype(np.float64) - exact) <= lim).all()
            assert abs(exact[lags.index(1)] / var - R.AR1_PHI).max() < 0.25 or second is not None
