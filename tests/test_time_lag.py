"""
CPU tests of the lagged-covariance functions of DLWP.verify on numpy inputs (the float64 host path): lag_covariance,
lag_correlation, autocorrelation, lag_regression, decorrelation_time, effective_sample_size.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time_lag_ref as R         # noqa: E402

from DLWP import verify          # noqa: E402
from DLWP.labelled import Forecast  # noqa: E402


def _brute(a, b, lag, center=True):
    """the covariance of two 1-d series at one lag with plain loops: (value, pairs)"""
    T = len(a)
    ma = np.nanmean(a) if center else 0.0
    mb = np.nanmean(b) if center else 0.0
    s, n = 0.0, 0
    for t in range(T):
        if 0 <= t + lag < T and not np.isnan(a[t]) and not np.isnan(b[t + lag]):
            s += (a[t] - ma) * (b[t + lag] - mb)
            n += 1
    return (s / n if n else np.nan), n


def _series(seed=0, T=60, E=4, nan=True):
    rng = np.random.default_rng(seed)
    a = R.ar1(rng, T, E, std=3.0, offset=10.0).astype(np.float64)
    b = R.ar1(rng, T, E, std=2.0, offset=-4.0).astype(np.float64)
    if nan:
        a[rng.random((T, E)) < 0.05] = np.nan
        b[rng.random((T, E)) < 0.05] = np.nan
    return a, b


def test_covariance_against_brute_force():
    a, b = _series(1)
    for second, lags in ((None, 5), (b, 5), (b[:, 0], [-7, -4, -1, 2, 5])):
        for center in ('mean', None):
            got, cnt = verify.lag_covariance(a, second, lags, center=center, return_count=True)
            lg = np.arange(0 if second is None else -5, 6) if isinstance(lags, int) else np.array(lags)
            assert got.shape == (len(lg), 4) and cnt.dtype == np.int32
            for i, l in enumerate(lg):
                for e in range(4):
                    bb = a[:, e] if second is None else (second if second.ndim == 1 else second[:, e])
                    want, n = _brute(a[:, e], bb, int(l), center == 'mean')
                    assert cnt[i, e] == n and abs(got[i, e] - want) <= 1e-12 * max(1.0, abs(want))


def test_axis_labels_and_lag_dim():
    a, b = _series(2, T=30, E=6, nan=False)
    fa = Forecast(a.T.reshape(2, 3, 30), ('lat', 'lon', 'time'), {'time': np.arange(30) * 6, 'lat': np.array([10., 20.])}, name='z')
    got, cnt = verify.lag_covariance(fa, lags=[-2, 0, 2], return_count=True)
    assert got.dims == ('lat', 'lon', 'lag') == cnt.dims and np.array_equal(got.coords['lag'], [-2, 0, 2])
    assert np.array_equal(got.coords['lat'], [10., 20.]) and got.name == 'lag_covariance' and cnt.name == 'lag_covariance_count'
    plain = verify.lag_covariance(a, lags=[-2, 0, 2])
    assert np.allclose(np.moveaxis(got.values, 2, 0).reshape(3, 6), plain, rtol=1e-13, atol=0)
    assert np.array_equal(got.values, verify.lag_covariance(fa.values, lags=[-2, 0, 2], axis=2))
    assert verify.autocorrelation(fa, 3).dims == ('lat', 'lon', 'lag')
    assert verify.decorrelation_time(fa, 5).dims == ('lat', 'lon') and verify.effective_sample_size(fa).dims == ('lat', 'lon')
    idx = a[:, 0]
    slope = verify.lag_regression(idx, fa, 2)
    assert slope.dims == ('lat', 'lon', 'lag') and np.array_equal(slope.coords['lag'], [-2, -1, 0, 1, 2])


def test_pure_cosine_over_whole_periods():
    """x_t = A cos(2 pi t / P) over whole periods: the biased autocovariance is A^2 / 2 cos(2 pi l / P) (1 - l / T) up to the
    end effect of the finite sum, exactly A^2 / 2 cos(2 pi l / P) for the circular estimator; with norm='pairs' the sum over the T - l
    pairs is A^2 / 2 ((T - l) cos(2 pi l / P) + the closed sum of cos(2 pi (2 t + l) / P) over the pairs) / (T - l)"""
    A, P, T = 3.0, 12, 120
    t = np.arange(T)
    x = A * np.cos(2 * np.pi * t / P)[:, None]
    lags = np.arange(0, 25)
    got = verify.lag_covariance(x, lags=lags, norm='biased')[:, 0]
    pairs = verify.lag_covariance(x, lags=lags, norm='pairs')[:, 0]
    for l in lags:
        tt = t[:T - l]
        closed = A * A / 2 * ((T - l) * np.cos(2 * np.pi * l / P) + np.cos(2 * np.pi * (2 * tt + l) / P).sum())
        assert abs(pairs[l] - closed / (T - l)) < 1e-12 and abs(got[l] - closed / T) < 1e-12
    # at the lags that are multiples of half a period the second sum vanishes: A^2 / 2 cos(2 pi l / P) (1 - l / T)
    for l in (0, 6, 12, 18, 24):
        assert abs(got[l] - A * A / 2 * np.cos(2 * np.pi * l / P) * (1 - l / T)) < 1e-12
    r = verify.autocorrelation(x, 24)[:, 0]
    assert r[0] == 1.0 and abs(r[12] - 1.0) < 1e-12 and abs(r[6] + 1.0) < 1e-12


def test_norm_missing_and_min_count():
    a, _ = _series(3)
    pairs, cnt = verify.lag_covariance(a, lags=4, return_count=True)
    biased = verify.lag_covariance(a, lags=4, norm='biased')
    assert np.allclose(biased, pairs * cnt / cnt[:1], rtol=1e-14, atol=0)
    with pytest.raises(ValueError, match='lag_covariance'):
        verify.lag_covariance(a, lags=[1, 2], norm='biased')
    prop = verify.lag_covariance(a, lags=4, missing='propagate')
    T = a.shape[0]
    complete = cnt == (T - np.arange(5))[:, None]
    assert np.array_equal(np.isnan(prop), ~complete) and np.array_equal(prop[complete], pairs[complete]) and (~complete).any()
    few = verify.lag_covariance(a[:8], lags=[1, 3, 5, 7, 9], min_count=3)
    n = verify.lag_covariance(a[:8], lags=[1, 3, 5, 7, 9], return_count=True)[1]
    assert np.array_equal(np.isnan(few), n < 3) and (n[4] == 0).all() and (n[3] <= 1).all() and (n[0] >= 3).any()
    raw = verify.lag_covariance(a, lags=[0], center=None)
    assert np.allclose(raw[0], np.nanmean(a * a, axis=0), rtol=1e-14)


def test_correlation_forms():
    a, b = _series(4)
    r = verify.lag_correlation(a, b, 3)
    c = verify.lag_covariance(a, b, 3)
    va, vb = verify.lag_covariance(a, lags=[0]), verify.lag_covariance(b, lags=[0])
    assert np.allclose(r, c / np.sqrt(va * vb), rtol=1e-14) and (np.abs(r) <= 1.05).all()
    # the autocorrelation divides by lag 0 of the same call; without lag 0 among the lags it is computed and dropped
    full = verify.lag_correlation(a, lags=[0, 1, 2, 3])
    part = verify.lag_correlation(a, lags=[2, 3])
    assert (full[0] == 1.0).all() and part.shape == (2, 4) and np.allclose(part, full[2:], rtol=1e-14)
    assert np.array_equal(verify.autocorrelation(a, 3), full)
    ri = verify.lag_correlation(a, b[:, 1], [0, 1])
    ci = verify.lag_covariance(a, b[:, 1], [0, 1])
    assert np.allclose(ri, ci / np.sqrt(va * verify.lag_covariance(b[:, 1], lags=[0])), rtol=1e-14)
    const = np.ones((10, 2))
    assert np.isnan(verify.autocorrelation(const, 2)).all()


def test_lag_regression_against_brute_force():
    a, b = _series(5, nan=False)
    idx = b[:, 0]
    slope, corr = verify.lag_regression(idx, a, [-3, -1, 1, 3], return_correlation=True)
    vi = _brute(idx, idx, 0)[0]
    for i, l in enumerate([-3, -1, 1, 3]):
        for e in range(4):
            c = _brute(idx, a[:, e], l)[0]                  # index[t] with x[t + l]
            assert abs(slope[i, e] - c / vi) < 1e-12
            assert abs(corr[i, e] - c / np.sqrt(vi * _brute(a[:, e], a[:, e], 0)[0])) < 1e-12
    # the regression of a shifted copy of the index peaks at the shift with slope 1
    x = np.zeros((60, 1))
    x[5:, 0] = idx[:-5]
    s = verify.lag_regression(idx[:-5], x[5:], 0)
    assert abs(s[0, 0] - 1.0) < 1e-12
    assert np.argmax(verify.lag_regression(idx, x, 8)[:, 0]) == 8 + 5


def test_effective_sample_size_against_its_formulas():
    rng = np.random.default_rng(6)
    x = R.ar1(rng, 400, 5).astype(np.float64)
    x[rng.random(x.shape) < 0.02] = np.nan
    r, cnt = verify.autocorrelation(x, 10, return_count=True)
    n = cnt[0].astype(np.float64)
    ar1 = verify.effective_sample_size(x)
    assert np.allclose(ar1, np.clip(n * (1 - r[1]) / (1 + r[1]), 1, n), rtol=1e-14)
    k = np.arange(1, 11)[:, None]
    tot = verify.effective_sample_size(x, method='sum', max_lag=10)
    assert np.allclose(tot, np.clip(n / (1 + 2 * ((1 - k / n) * r[1:]).sum(axis=0)), 1, n), rtol=1e-13)
    assert (ar1 < n / 4).all() and (ar1 > n / 20).all()    # phi = 0.8: n / 9
    # white noise: close to n, clipped at n; a pair: the product of the two lag-1 autocorrelations
    w = rng.standard_normal((400, 3))
    assert (verify.effective_sample_size(w) <= 400).all() and (verify.effective_sample_size(w) > 300).all()
    y = R.ar1(rng, 400, 5).astype(np.float64)
    ry = verify.autocorrelation(y, 1)
    pair = verify.effective_sample_size(x, y)
    nb = verify.lag_covariance(x, y, [0], return_count=True)[1][0].astype(np.float64)
    assert np.allclose(pair, np.clip(nb * (1 - r[1] * ry[1]) / (1 + r[1] * ry[1]), 1, nb), rtol=1e-14)
    assert np.isnan(verify.effective_sample_size(np.full((5, 2), np.nan))).all()


def test_decorrelation_time_interpolates_and_gives_inf():
    # r_k = phi^k exactly would need an infinite series; build the autocorrelation by hand instead through a known series:
    # a cosine of period 40 has r_k close to cos(2 pi k / 40): it crosses exp(-1) between k = 7 and k = 8
    t = np.arange(400)
    x = np.cos(2 * np.pi * t / 40)[:, None]
    r = verify.autocorrelation(x, 12)[:, 0]
    thr = np.exp(-1.0)
    k = int(np.argmax(r[1:] < thr)) + 1
    want = (k - 1) + (r[k - 1] - thr) / (r[k - 1] - r[k])
    got = verify.decorrelation_time(x, 12)
    assert got.shape == (1,) and abs(got[0] - want) < 1e-12 and k - 1 < got[0] < k
    assert np.isinf(verify.decorrelation_time(x, 3)[0])         # it does not cross within 3 lags
    assert abs(verify.decorrelation_time(x, 12, threshold=0.5)[0] - 40 / 6) < 0.2
    both = np.concatenate([x, np.full((400, 1), np.nan)], axis=1)
    d = verify.decorrelation_time(both, 12)
    assert abs(d[0] - want) < 1e-12 and np.isnan(d[1])


def test_every_value_error_names_its_function():
    a, b = _series(7)
    bad = [
        ('lag_covariance', lambda: verify.lag_covariance(a, lags=[0, 2, 3])),
        ('lag_covariance', lambda: verify.lag_covariance(a, lags=[2, 1])),
        ('lag_covariance', lambda: verify.lag_covariance(a, lags=[])),
        ('lag_covariance', lambda: verify.lag_covariance(a, lags=[0.5])),
        ('lag_covariance', lambda: verify.lag_covariance(a, lags=-1)),
        ('lag_covariance', lambda: verify.lag_covariance(a, lags=2000)),
        ('lag_covariance', lambda: verify.lag_covariance(a, b[:-1], 1)),
        ('lag_covariance', lambda: verify.lag_covariance(a, lags=1, center='median')),
        ('lag_covariance', lambda: verify.lag_covariance(a, lags=1, missing='drop')),
        ('lag_covariance', lambda: verify.lag_covariance(a, lags=1, min_count=0)),
        ('lag_covariance', lambda: verify.lag_covariance(a, lags=1, norm='unbiased')),
        ('lag_correlation', lambda: verify.lag_correlation(a, lags=[3, 1])),
        ('lag_correlation', lambda: verify.lag_correlation(a, b[:, :2], 1)),
        ('autocorrelation', lambda: verify.autocorrelation(a, -1)),
        ('autocorrelation', lambda: verify.autocorrelation(a, 1.5)),
        ('lag_regression', lambda: verify.lag_regression(b[:-1, 0], a, 1)),
        ('lag_regression', lambda: verify.lag_regression(b, a, 1)),
        ('lag_regression', lambda: verify.lag_regression(b[:, 0], a, [1, 3, 4])),
        ('decorrelation_time', lambda: verify.decorrelation_time(a, 0)),
        ('decorrelation_time', lambda: verify.decorrelation_time(a, 5, threshold=1.5)),
        ('effective_sample_size', lambda: verify.effective_sample_size(a, method='bartlett')),
        ('effective_sample_size', lambda: verify.effective_sample_size(a, method='sum')),
        ('effective_sample_size', lambda: verify.effective_sample_size(a, max_lag=3)),
        ('effective_sample_size', lambda: verify.effective_sample_size(a, b[:, :2])),
    ]
    for name, call in bad:
        with pytest.raises(ValueError, match=name):
            call()
    with pytest.raises(ValueError):
        verify.lag_covariance(Forecast(a, ('time', 'x'), {}), lags=1, axis='lead')


def test_host_twin_matches_the_reference_on_float32_data():
    """_time_lag_host is the float64 twin of the device kernel: on float32 data with the float32 centre it meets the bit-exact
    reference to float32 rounding"""
    rng = np.random.default_rng(8)
    a, b = R.make_series(rng, 600, 7, 'one percent')
    lags = list(range(-5, 6))
    ca, cb = R.centre(a), R.centre(b)
    want, wn = R.reference(a, b, lags, ca, cb)
    got, n = verify._time_lag_host(a, b, lags, 0, ca.astype(np.float64), cb.astype(np.float64))
    assert np.array_equal(n, wn) and np.abs(got - want).max() <= 2.0 ** -22 * np.abs(want).max()
