"""
CPU tests of the reference of the least-squares fit (time_regression_ref.py): the vectorised restatement against the scalar one
bit for bit, against numpy.linalg.lstsq in fp64 on the present rows of every kept column, and the planner's table closed over
its cases.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time_regression_ref as R      # noqa: E402

LSTSQ_CASES = ((4, 40), (6, 97), (10, 365), (16, 1100), (16, 40), (10, 513))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize('K,T,S', ((1, 9, 4), (2, 21, 8), (3, 40, 8), (5, 33, 0), (10, 40, 8), (16, 50, 16), (4, 3, 8), (4, 4, 8)))
def test_vectorised_against_scalar_restatement(K, T, S):
    rng = np.random.default_rng(K * 100 + T)
    E = 23
    x = R.make_series(rng, T, E, K)
    b = R.harmonic_basis(T, K)
    for mode in (R.SKIP, R.PROPAGATE):
        for mc in (K, K + 3):
            coef, n, _ = R.fit_ref(x, b, mode, mc, slab_rows=S)
            for e in range(E):
                bits, ne = R.fit_scalar(x[:, e], b, mode, mc, slab_rows=S)
                assert ne == n[e]
                assert list(_bits(coef[:, e])) == bits, 'K %d T %d element %d mode %d' % (K, T, e, mode)
    # complete data: every column is kept in both modes
    xc = R.make_series(rng, T, 5, hostile=False)
    coef, n, sing = R.fit_ref(xc, b, R.PROPAGATE, slab_rows=S)
    assert np.all(n == T) and (T < K or (not sing.any() and np.isfinite(coef).all()))


@pytest.mark.parametrize('K,T', LSTSQ_CASES)
def test_against_lstsq_on_the_present_rows(K, T):
    rng = np.random.default_rng(K + T)
    E = 48
    x = R.make_series(rng, T, E, K)
    b = R.harmonic_basis(T, K)
    coef, n, sing = R.fit_ref(x, b)
    bd = b.astype(np.float64)
    worst, kept = 0., 0
    for e in range(E):
        if n[e] < K:
            assert np.all(_bits(coef[:, e]) == R.QNAN)
            continue
        assert not sing[e], 'a column with %d >= K present rows was flagged singular' % n[e]
        ok = ~np.isnan(x[:, e])
        if not np.all(np.isfinite(x[ok, e])):
            assert np.all(_bits(coef[:, e]) == R.QNAN)         # an infinity is a value: the coefficients are not finite
            continue
        want = np.linalg.lstsq(bd[ok], x[ok, e].astype(np.float64), rcond=None)[0]
        scale = np.abs(want).max()
        err = np.abs(coef[:, e].astype(np.float64) - want).max() / (R.U * scale)
        worst = max(worst, err)
        kept += 1
        assert err <= 2., 'K %d T %d element %d: %.3f x 2^-24 max|coef|' % (K, T, e, err)
    print('K %d T %d: worst %.3f x 2^-24 x max|coef| over %d columns' % (K, T, worst, kept))
    assert kept > E // 2


def test_collinear_and_short():
    rng = np.random.default_rng(1)
    x = R.make_series(rng, 30, 7, hostile=False)
    b = R.harmonic_basis(30, 4)
    b[:, 3] = b[:, 1]
    coef, n, sing = R.fit_ref(x, b)
    assert sing.all() and np.all(_bits(coef) == R.QNAN) and np.all(n == 30)
    coef, n, _ = R.fit_ref(x[:3], R.harmonic_basis(3, 4))
    assert np.all(_bits(coef) == R.QNAN) and np.all(n == 3)


def test_apply_ref():
    rng = np.random.default_rng(2)
    x = R.make_series(rng, 40, 9, 4)
    b = R.harmonic_basis(40, 4)
    coef, n, _ = R.fit_ref(x, b)
    fit, res = R.apply_ref(b, coef), R.apply_ref(b, coef, x)
    bad = np.isnan(coef).any(axis=0)
    assert np.all(_bits(fit[:, bad]) == R.QNAN) and np.isfinite(fit[:, ~bad]).all()
    assert np.array_equal(np.isnan(res), np.isnan(x) | bad[None, :])
    ok = ~np.isnan(res) & np.isfinite(x)
    assert np.allclose((x.astype(np.float64) - fit)[ok], res[ok], rtol=0, atol=1e-4)


def test_plan_closed_over_its_cases():
    for K in range(1, R.MAX_TERMS + 1):
        cls = R.term_class(K)
        assert cls in (1, 2, 4, 8, 16) and cls >= K and (cls == 1 or cls // 2 < K)
    # (T, K, inner, vec_ok, slab_rows, split, gram) -> (split, gram, class, chunk, grid, slab rows)
    table = {
        (1100, 10, 1028, True, 0, -1, -1): (1, 0, 16, 1, (15, 1), 512),
        (1100, 8, 1028, True, 0, -1, -1): (1, 0, 8, 4, (6, 1), 512),
        (1100, 8, 1028, False, 0, -1, -1): (1, 0, 8, 1, (15, 1), 512),
        (512, 8, 1028, True, 0, -1, -1): (0, 0, 8, 4, (2, 1), 512),
        (513, 2, 13824, True, 0, -1, 1): (1, 1, 2, 4, (28, 1), 512),
        (40, 3, 5, False, 8, -1, -1): (1, 0, 4, 1, (5, 1), 8),
        (40, 3, 5, False, 8, 0, -1): (0, 0, 4, 1, (1, 1), 8),
        (0, 1, 256, True, 0, -1, -1): (0, 0, 1, 4, (1, 1), 512),
        (20000, 16, 600000, True, 0, -1, -1): (0, 0, 16, 1, (2344, 1), 512),
        (20000, 4, 600000, True, 0, -1, -1): (0, 0, 4, 4, (586, 1), 512),
        (20000, 4, 400000, True, 0, -1, -1): (1, 0, 4, 4, (15640, 1), 512),
        (100, 4, 0, True, 0, -1, -1): (0, 0, 4, 4, (0, 0), 512),
        (2000, 1, 256 * 4 * 70000, True, 1000, 1, -1): (1, 0, 1, 4, (65536, 3), 1000),
    }
    for args, want in table.items():
        assert R.plan(*args) == want, args
    assert R.plan(10, 17, 4, True) is None and R.plan(10, 0, 4, True) is None
