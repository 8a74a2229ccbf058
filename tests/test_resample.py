"""
CPU tests of DLWP.verify.resample on the host path (the float64 twin): the draw table, the replicate means against the numpy
restatement of tests/resample_ref.py, the statistics, the interval of a Gaussian series against its analytic standard error,
the paired difference, labels, every error, and block_length='auto' on an AR(1) series.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import resample_ref as R                                                  # noqa: E402

from DLWP import verify                                                   # noqa: E402
from DLWP.labelled import Forecast                                        # noqa: E402


def test_the_draw_table_is_deterministic_per_seed():
    a = verify.bootstrap_starts(50, 20, 4, seed=3)
    assert a.shape == (20, 13) and a.dtype == np.int32 and a.min() >= 0 and a.max() < 50
    assert np.array_equal(a, verify.bootstrap_starts(50, 20, 4, seed=3))
    assert not np.array_equal(a, verify.bootstrap_starts(50, 20, 4, seed=4))
    want = np.random.Generator(np.random.PCG64(3)).integers(0, 50, size=(20, 13), dtype=np.int64)
    assert np.array_equal(a, want)
    m = verify.bootstrap_starts(50, 400, 7, circular=False, seed=1)
    assert m.max() == 43 and m.min() == 0                    # moving blocks: 0 .. T-L, none wraps
    assert verify.bootstrap_starts(50, 400, 7, seed=1).max() > 43
    assert verify.bootstrap_starts(10, 3, 4, n_draw=21).shape == (3, 6)
    assert verify.bootstrap_starts(10, 1000).shape == (1000, 10)


@pytest.mark.parametrize('L', [1, 3, 12])
@pytest.mark.parametrize('missing,min_count', [('skip', 1), ('skip', 11), ('propagate', 1)])
def test_the_host_twin_is_the_definition_before_its_rounding(L, missing, min_count):
    T, E, B = 12, 10, 9
    rng = np.random.default_rng(L)
    x = R.make_series(rng, T, E, 'one percent')
    x[3:6, 4] = np.nan
    st = R.make_starts(rng, T, B, L)
    got, n = verify.bootstrap_mean(x, n_resamples=B, block_length=L, starts=st, missing=missing, min_count=min_count, return_count=True)
    want, wn = R.reference(x, st, L, None, R.SKIP if missing == 'skip' else R.PROPAGATE, min_count)
    assert got.dtype == np.float64 and n.dtype == np.int32 and np.array_equal(n, wn)
    assert np.array_equal(R.bits(got.astype(np.float32)), R.bits(want))
    # column 4 misses three of its twelve times: some resample draws one of them, and hardly one draws eleven others
    assert np.isnan(got[:, 4]).any() == (missing == 'propagate' or min_count > 1) and not np.isnan(got[:, :4]).all()


def test_starts_override_the_draw_and_the_seed_decides_otherwise():
    x = R.make_series(np.random.default_rng(0), 30, 4)
    st = verify.bootstrap_starts(30, 25, 2, seed=11)
    a = verify.bootstrap_mean(x, n_resamples=25, block_length=2, seed=11)
    assert np.array_equal(a, verify.bootstrap_mean(x, n_resamples=3, block_length=2, seed=99, starts=st))
    assert np.array_equal(a, verify.bootstrap_mean(x, n_resamples=25, block_length=2, seed=11))
    assert not np.array_equal(a, verify.bootstrap_mean(x, n_resamples=25, block_length=2, seed=12))
    assert a.shape == (25, 4)


def test_a_constant_series_and_whole_circular_blocks_have_no_spread():
    c = np.full((20, 3), 7.25, dtype=np.float32)
    assert np.array_equal(verify.bootstrap_mean(c, n_resamples=50, block_length=3), np.full((50, 3), 7.25))
    x = R.make_series(np.random.default_rng(2), 20, 3)
    iv = verify.bootstrap_interval(x, n_resamples=60, block_length=20, return_replicates=True)       # L = T, circular: a rotation
    full = x.astype(np.float64).mean(axis=0)
    assert np.abs(iv.replicates - full).max() <= 1e-12 * np.abs(full).max()
    assert (iv.standard_error <= 1e-12 * np.abs(full)).all() and np.allclose(iv.low, full, rtol=1e-12) and np.allclose(iv.high, full, rtol=1e-12)
    assert iv.block_length == 20 and iv.n_resamples == 60 and iv.level == 0.95 and iv.p_value is None


def test_the_interval_of_a_gaussian_series_holds_its_analytic_standard_error():
    """T = 400 independent N(1, sigma^2) times, sigma = 2, B = 2000, 16 columns, a fixed seed.  The bootstrap standard error
    estimates s sqrt((T - 1) / T) / sqrt(T) with s the sample standard deviation: relative error 1 / sqrt(2 T) = 3.5 % from s and
    1 / sqrt(2 B) = 1.6 % from the Monte-Carlo draw, together 3.9 %; three of that, 12 %, is the margin.  A percentile limit at
    p = 0.025 has the Monte-Carlo error sqrt(p (1 - p) / B) / density = 0.0035 / (0.0584 / se) = 6 % of se, the half-width
    1.96 se so 3 % (the two limits independent: 2.2 %) on top of the 3.5 % of s: three of 4.1 % is 12.5 %."""
    T, E, B, sigma = 400, 16, 2000, 2.0
    x = np.random.default_rng(42).standard_normal((T, E)) * sigma + 1.0
    iv = verify.bootstrap_interval(x, n_resamples=B, seed=7)
    se = sigma / np.sqrt(T)
    assert np.abs(iv.standard_error / se - 1.).max() < 0.12
    assert np.abs((iv.high - iv.low) / (2 * 1.959964 * se) - 1.).max() < 0.125
    assert np.array_equal(iv.estimate, x.mean(axis=0)) or np.allclose(iv.estimate, x.mean(axis=0), rtol=1e-14)
    assert (iv.low < iv.estimate).all() and (iv.estimate < iv.high).all()
    # the true mean lies inside 95 % intervals about 95 % of the time: of 16 columns at most 3 miss (probability of more: 0.7 %)
    assert ((iv.low > 1.0) | (iv.high < 1.0)).sum() <= 3


def test_the_statistics_are_the_formulas_of_the_replicate_means():
    T, E, B = 40, 5, 30
    rng = np.random.default_rng(5)
    p, q, r = (rng.random((T, E)) + 0.5 for _ in range(3))
    st = verify.bootstrap_starts(T, B, 4, seed=2)
    m = [verify.bootstrap_mean(v, block_length=4, starts=st) for v in (p, q, r)]
    want = {'mean': ((p,), m[0]), 'rmse': ((p,), np.sqrt(m[0])), 'ratio': ((p, q), m[0] / m[1]),
            'correlation': ((p, q, r), m[0] / np.sqrt(m[1] * m[2])), 'skill': ((p, q), 1. - m[0] / m[1])}
    for stat, (xs, rep) in want.items():
        iv = verify.bootstrap_interval(xs if len(xs) > 1 else xs[0], stat, level=0.9, block_length=4, starts=st, return_replicates=True)
        assert np.array_equal(iv.replicates, rep), stat
        assert np.allclose(iv.low, np.quantile(rep, 0.05, axis=0), rtol=1e-14) and np.allclose(iv.high, np.quantile(rep, 0.95, axis=0), rtol=1e-14)
        assert np.allclose(iv.standard_error, rep.std(axis=0, ddof=1), rtol=1e-12)
        assert iv.level == 0.9 and iv.n_resamples == B
    full = {'rmse': np.sqrt(p.mean(0)), 'correlation': p.mean(0) / np.sqrt(q.mean(0) * r.mean(0))}
    assert np.allclose(verify.bootstrap_interval(p, 'rmse', starts=st, block_length=4).estimate, full['rmse'], rtol=1e-14)
    assert np.allclose(verify.bootstrap_interval((p, q, r), 'correlation', starts=st, block_length=4).estimate, full['correlation'], rtol=1e-14)
    iv = verify.bootstrap_interval((p, q), lambda a, b: a - 2. * b, starts=st, block_length=4, return_replicates=True)
    assert np.array_equal(iv.replicates, m[0] - 2. * m[1])


def test_the_paired_difference():
    T, E = 60, 4
    rng = np.random.default_rng(8)
    a = rng.random((T, E)) + 1.0
    same = verify.bootstrap_difference(a, a, n_resamples=100, block_length=3)
    assert not np.any(same.estimate) and np.array_equal(same.p_value, np.ones(E)) and not np.any(same.standard_error)
    b = a + 0.5 + 0.01 * rng.standard_normal((T, E))         # b is worse by far more than the noise: no replicate at or above 0
    d = verify.bootstrap_difference(a, b, n_resamples=100, block_length=3, return_replicates=True)
    assert (d.replicates < 0).all() and not np.any(d.p_value) and (d.high < 0).all()
    st = verify.bootstrap_starts(T, 100, 3)
    assert np.array_equal(d.replicates, verify.bootstrap_mean(a, block_length=3, starts=st) - verify.bootstrap_mean(b, block_length=3, starts=st))
    assert np.allclose(d.estimate, (a - b).mean(axis=0), rtol=1e-12)
    # the shared draw table cancels what the systems share: far narrower than the two intervals apart
    assert (d.standard_error < 0.05 * verify.bootstrap_interval(a, n_resamples=100, block_length=3).standard_error).all()
    c = a + 0.02 * rng.standard_normal((T, E))                # a difference inside the noise: a p value strictly between
    p = verify.bootstrap_difference((a, a), (c, a), 'ratio', n_resamples=200).p_value
    assert ((p > 0) & (p <= 1)).all()
    rep = verify.bootstrap_difference(a, c, n_resamples=200, return_replicates=True)
    want = np.minimum(1., 2. * np.minimum((rep.replicates <= 0).mean(axis=0), (rep.replicates >= 0).mean(axis=0)))
    assert np.array_equal(rep.p_value, want)


def test_labels_and_dims():
    T = 10
    x = R.make_series(np.random.default_rng(3), T, 12).reshape(T, 3, 4)
    f = Forecast(np.moveaxis(x, 0, 1), ('varlev', 'time', 'lat'), {'varlev': np.array(['z', 't', 'q']), 'time': np.arange(T) * 6,
                                                                   'lat': np.linspace(-60, 60, 4)}, 'err')
    m, n = verify.bootstrap_mean(f, n_resamples=7, block_length=2, return_count=True)
    assert m.dims == ('varlev', 'resample', 'lat') == n.dims and m.shape == (3, 7, 4) and m.name == 'bootstrap_mean'
    assert np.array_equal(m.coords['resample'], np.arange(7)) and np.array_equal(m.coords['lat'], f.coords['lat'])
    assert np.array_equal(m.values, np.moveaxis(verify.bootstrap_mean(x, n_resamples=7, block_length=2), 0, 1))
    iv = verify.bootstrap_interval(f, 'rmse', n_resamples=7, block_length=2, return_replicates=True)
    for field in (iv.estimate, iv.low, iv.high, iv.standard_error):
        assert field.dims == ('varlev', 'lat') and field.shape == (3, 4) and list(field.coords['varlev']) == ['z', 't', 'q']
    assert iv.replicates.dims == ('varlev', 'resample', 'lat') and iv.estimate.name == 'bootstrap_interval_estimate'
    d = verify.bootstrap_difference(f, f, n_resamples=7)
    assert d.p_value.dims == ('varlev', 'lat') and np.array_equal(d.p_value.values, np.ones((3, 4)))
    assert verify.bootstrap_mean(x, axis=1, n_resamples=5).shape == (T, 5, 4)
    assert verify.bootstrap_mean(f, axis='lat', n_resamples=5).dims == ('varlev', 'time', 'resample')


def test_every_error():
    x = np.zeros((8, 3))
    for kw in (dict(level=0.), dict(level=1.), dict(level=1.5), dict(level='wide'), dict(n_resamples=0), dict(block_length=0),
               dict(block_length=9), dict(block_length='long'), dict(block_length=2.5), dict(missing='drop'), dict(min_count=0),
               dict(statistic='median'), dict(statistic='ratio'), dict(starts=np.zeros((4, 3), dtype=np.int64)),
               dict(starts=np.zeros((4, 8))), dict(starts=np.zeros(8, dtype=np.int64)), dict(axis=2), dict(axis='time')):
        with pytest.raises(ValueError):
            verify.bootstrap_interval(x, **kw)
    for bad in (np.full((4, 8), 8), np.full((4, 8), -1)):
        with pytest.raises(IndexError):
            verify.bootstrap_interval(x, starts=bad)
        with pytest.raises(IndexError):
            verify.bootstrap_mean(x, starts=bad)
    with pytest.raises(ValueError):
        verify.bootstrap_interval((x, np.zeros((8, 4))), 'ratio')
    with pytest.raises(ValueError):
        verify.bootstrap_interval((x, x), 'mean')
    with pytest.raises(ValueError):
        verify.bootstrap_mean((x, x))
    with pytest.raises(ValueError):
        verify.bootstrap_difference(x, np.zeros((8, 4)))
    with pytest.raises(ValueError):
        verify.bootstrap_difference(x, (x, x), 'mean')
    with pytest.raises(ValueError):
        verify.bootstrap_mean(np.zeros((0, 3)))
    for kw in (dict(n_times=0), dict(n_times=5, block_length=6), dict(n_times=5, n_resamples=0), dict(n_times=5, n_draw=0)):
        with pytest.raises(ValueError):
            verify.bootstrap_starts(**kw)


def test_block_length_auto_on_an_ar1_series():
    """phi = 0.6, T = 2000, 200 columns.  ESS = n (1 - r1) / (1 + r1), so L = ceil((1 + r1) / (1 - r1)).  r1 of a column has the
    standard deviation sqrt((1 - phi^2) / T) = 0.018 and the bias -(1 + 4 phi) / T = -0.0017; the median of 200 columns lies
    within 0.02 of phi with a wide margin, and r1 in [0.58, 0.62] gives (1 + r1) / (1 - r1) in [3.76, 4.27]: L is 4 or 5."""
    T, E, phi = 2000, 200, 0.6
    rng = np.random.default_rng(6)
    x = rng.standard_normal((T, E))
    for t in range(1, T):
        x[t] += phi * x[t - 1]
    ess = np.median(verify.effective_sample_size(x))
    assert T * 0.38 / 1.62 <= ess <= T * 0.42 / 1.58
    iv = verify.bootstrap_interval(x, n_resamples=4, block_length='auto')
    assert iv.block_length == int(np.ceil(T / ess)) and iv.block_length in (4, 5)
    assert verify.bootstrap_mean(x, n_resamples=4, block_length='auto').shape == (4, E)
    # white noise: one time a block; a constant series has no autocorrelation to speak of: 1
    assert verify.bootstrap_interval(rng.standard_normal((500, 50)), n_resamples=2, block_length='auto').block_length <= 2
    assert verify.bootstrap_interval(np.ones((20, 2)), n_resamples=2, block_length='auto').block_length == 1
