"""
Climatologies on the host path (reference DLWP/verify.py:167-214, 426-456): `daily_climatology`, `daily_climo_time_series`,
`monthly_climo_error`, `ClimatologyLookup` and `TimeSeriesEstimator.climatology` against tests/golden/g15_climatology.npz
(an fp64 restatement whose calendar quantities come from pandas, tests/golden/gen_golden_climatology.py).  No device work.

The accuracy bound of a group mean is derived, not tuned: against the fp64 expectation m of n non-NaN members,
|r - m| <= 2**-24 |m| + n 2**-52 mean|x| -- one rounding to fp32 plus the worst case of an fp64 running sum.
"""
import json
import os

import numpy as np
import pytest

from DLWP.model.extensions import Forecast

DIMS = ('time', 'x0', 'x1', 'x2', 'varlev')


@pytest.fixture(scope='module')
def g(golden_dir):
    return np.load(os.path.join(golden_dir, 'g15_climatology.npz'))


def labelled(values, times, dims=DIMS, lat=None):
    coords = {d: (times if d in ('time', 'sample') else np.arange(values.shape[i])) for i, d in enumerate(dims)}
    out = Forecast(values, list(dims), coords)
    if lat is not None:
        out.lat = Forecast(lat, ['x0', 'x1', 'x2'], {d: np.arange(s) for d, s in zip(('x0', 'x1', 'x2'), lat.shape)})
    return out


def check_group_mean(got, want, data, keys, uniq):
    """got (K, ...) fp32 against the fp64 expectation under the derived bound; NaN and inf in the same places"""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.isinf(got), np.isinf(want)) and np.array_equal(got[np.isinf(want)], want[np.isinf(want)])
    for i, k in enumerate(uniq):
        x = data[keys == k].astype(np.float64)
        ok = ~np.isnan(x)
        n = ok.sum(axis=0)
        with np.errstate(invalid='ignore', divide='ignore'):
            mean_abs = np.where(ok, np.abs(x), 0.).sum(axis=0) / np.maximum(n, 1)
        fin = np.isfinite(want[i])
        bound = 2. ** -24 * np.abs(want[i][fin]) + n[fin] * 2. ** -52 * mean_abs[fin]
        err = np.abs(got[i][fin].astype(np.float64) - want[i][fin])
        assert (err <= bound).all(), (k, float((err / bound).max()))


def test_calendar_keys_match_pandas_for_every_day_of_1999_to_2004(g):
    from DLWP.verify import calendar_keys
    assert len(g['cal_times']) == 2192 and {60, 366} <= set(g['cal_doy'].tolist())
    for unit in ('h', 's', 'ns'):
        t = g['cal_times'].astype('datetime64[%s]' % unit)
        d, m = calendar_keys(t), calendar_keys(t, 'month')
        assert d.dtype == np.int64 and np.array_equal(d, g['cal_doy']) and np.array_equal(m, g['cal_month'])
    assert np.array_equal(calendar_keys(g['times']), g['doy']) and np.array_equal(calendar_keys(g['times'], 'month'), g['month'])
    with pytest.raises(TypeError, match='datetime64'):
        calendar_keys(np.arange(4))
    with pytest.raises(ValueError, match="'dayofyear' or 'month'"):
        calendar_keys(g['times'], 'week')


@pytest.mark.parametrize('layout', ['channels_last', 'channels_first', 'time_inside'])
@pytest.mark.parametrize('by', ['dayofyear', 'month'])
def test_daily_climatology_matches_golden(g, layout, by):
    from DLWP.verify import daily_climatology
    data, times = g['data'], g['times']
    keys, uniq, want = (g['doy'], g['doy_keys'], g['doy_mean']) if by == 'dayofyear' else (g['month'], g['month_keys'],
                                                                                              g['month_mean'])
    perm = {'channels_last': (0, 1, 2, 3, 4), 'channels_first': (0, 4, 1, 2, 3), 'time_inside': (1, 2, 0, 3, 4)}[layout]
    src = labelled(np.ascontiguousarray(data.transpose(perm)), times, tuple(DIMS[p] for p in perm))
    out = daily_climatology(src, by=by) if by != 'dayofyear' else daily_climatology(src)
    assert out.dims == tuple(by if d == 'time' else d for d in src.dims)
    assert out.coords[by].dtype == np.int64 and np.array_equal(out.coords[by], uniq)
    assert np.array_equal(out.coords['x0'], np.arange(6))
    back = np.asarray(out.values).transpose(np.argsort(perm))
    check_group_mean(back, want, data, keys, uniq)


def test_daily_climatology_refusals(g):
    from DLWP.verify import daily_climatology
    src = labelled(g['data'], g['times'], ('sample',) + DIMS[1:])
    with pytest.raises(ValueError, match="no 'time' dimension"):
        daily_climatology(src)
    with pytest.raises(TypeError, match='datetime64'):
        daily_climatology(labelled(g['data'], np.arange(len(g['times']))))
    with pytest.raises(TypeError):
        daily_climatology(labelled(g['data'], g['times']), 'month')          # `by` is keyword-only


@pytest.mark.parametrize('lead', ['none', 'int', 'timedelta', 'float'])
def test_daily_climo_time_series_matches_golden(g, lead):
    from DLWP.verify import ClimatologyLookup, daily_climatology, daily_climo_time_series
    clim = daily_climatology(labelled(g['data'], g['times']))
    ts = g['ts_times']
    f_hour = {'none': None, 'int': g['ts_f_hour'], 'timedelta': g['ts_f_hour'].astype('timedelta64[h]'),
              'float': g['ts_f_hour'].astype(np.float64)}[lead]
    doy = g['ts_doy_none'] if lead == 'none' else g['ts_doy_lead']
    want = np.asarray(clim.values)[np.searchsorted(g['doy_keys'], doy)]
    out = daily_climo_time_series(clim, ts, f_hour)
    assert out.dims == (('time',) if lead == 'none' else ('f_hour', 'time')) + DIMS[1:]
    assert np.array_equal(out.coords['time'], ts)
    if lead != 'none':
        assert np.array_equal(out.coords['f_hour'], f_hour) and out.coords['f_hour'].dtype == f_hour.dtype
    assert out.values.dtype == np.float32 and np.array_equal(out.values, want, equal_nan=True)
    lazy = daily_climo_time_series(clim, ts, f_hour, lazy=True)
    assert isinstance(lazy, ClimatologyLookup) and lazy.shape == want.shape and lazy.dims == out.dims
    assert lazy.rows.dtype == np.int32 and np.array_equal(g['doy_keys'][lazy.rows], doy)
    assert np.array_equal(lazy.materialize().values, want, equal_nan=True)
    with pytest.raises(TypeError):
        daily_climo_time_series(clim, ts, f_hour, True)                      # `lazy` is keyword-only


def test_daily_climo_time_series_with_the_day_axis_inside(g):
    from DLWP.verify import daily_climatology, daily_climo_time_series
    src = labelled(np.ascontiguousarray(g['data'].transpose(1, 0, 2, 3, 4)), g['times'], ('x0', 'time', 'x1', 'x2', 'varlev'))
    clim = daily_climatology(src)
    out = daily_climo_time_series(clim, g['ts_times'], g['ts_f_hour'])
    assert out.dims == ('f_hour', 'x0', 'time', 'x1', 'x2', 'varlev')
    want = np.asarray(daily_climatology(labelled(g['data'], g['times'])).values)[np.searchsorted(g['doy_keys'], g['ts_doy_lead'])]
    assert np.array_equal(out.values, np.moveaxis(want, 2, 1), equal_nan=True)


def test_a_day_the_climatology_lacks_raises_keyerror_naming_it(g):
    from DLWP.verify import daily_climo_time_series
    part = labelled(g['given_dayofyear'], g['given_dayofyear_keys'], ('dayofyear',) + DIMS[1:])
    part.coords['dayofyear'] = g['given_dayofyear_keys']
    daily_climo_time_series(part, g['missing_day_times'][:1])
    for lazy in (False, True):
        with pytest.raises(KeyError, match=r'\b%d\b' % int(g['missing_day'])):
            daily_climo_time_series(part, g['missing_day_times'], lazy=lazy)
    with pytest.raises(ValueError, match="no 'dayofyear' dimension"):
        daily_climo_time_series(labelled(g['data'], g['times']), g['ts_times'])


def _climo_da(g, by, time_dim='time'):
    dims = tuple(by if d == time_dim else d for d in (time_dim,) + DIMS[1:])
    out = labelled(g['given_%s' % by], g['given_%s_keys' % by], dims)
    out.coords[by] = g['given_%s_keys' % by]
    return out


def run_monthly_case(g, c, wrap=lambda x: x, time_dim='time'):
    from DLWP.verify import monthly_climo_error
    by = 'dayofyear' if c['by_day_of_year'] else 'month'
    da = labelled(wrap(g['data']), g['times'], (time_dim,) + DIMS[1:], lat=g['lat'])
    climo = None
    if c['climo_da']:
        climo = _climo_da(g, by, time_dim)
        climo.values = wrap(climo.values)
    return monthly_climo_error(da, g['val_set'], n_fhour=c['n_fhour'], method=c['method'], climo_da=climo,
                               by_day_of_year=c['by_day_of_year'], weighted=c['weighted'])


def check_monthly(got, c):
    """the tolerances of the score tests for the same methods (tests/test_verify_scores.py: rtol 1e-5, no atol)"""
    if c['n_fhour'] is not None:
        assert isinstance(got, np.ndarray) and got.shape == (c['n_fhour'],) and (got == got[0]).all()
        got = got[0]
    else:
        assert isinstance(got, float)
        assert (type(got) is float) == (c['method'] != 'rmse')              # np.sqrt of a float is a np.float64 (:199)
    if c['method'] in ('acc', 'cos'):
        assert got == 0.
    else:
        np.testing.assert_allclose(got, c['value'], rtol=1e-5, atol=0.)


def test_monthly_climo_error_matches_every_golden_case(g):
    cases = json.loads(str(g['cases']))
    assert len(cases) == 40
    for c in cases:
        check_monthly(run_monthly_case(g, c), c)
    # 'sample' is preferred over 'time' as the time dimension
    check_monthly(run_monthly_case(g, cases[0], time_dim='sample'), cases[0])


def test_monthly_climo_error_anomaly_types_and_errors(g):
    from DLWP.verify import monthly_climo_error
    cases = json.loads(str(g['cases']))
    da = labelled(g['data'], g['times'], lat=g['lat'])
    for c in cases:
        if c['method'] != 'mae' or c['weighted']:
            continue
        by = 'dayofyear' if c['by_day_of_year'] else 'month'
        me, anomaly = monthly_climo_error(da, g['val_set'], method='mae', climo_da=_climo_da(g, by) if c['climo_da'] else None,
                                          by_day_of_year=c['by_day_of_year'], return_da=True)
        np.testing.assert_allclose(me, c['value'], rtol=1e-5, atol=0.)
        want = g[c['anomaly']]
        assert anomaly.dims == DIMS and np.array_equal(anomaly.coords['time'], g['val_set'])
        assert np.array_equal(np.isnan(anomaly.values), np.isnan(want))
        # the climatology is fp32 (one rounding of a value up to max|x|) and so is the anomaly (one more, of a smaller value)
        atol = 2. ** -23 * float(np.abs(g['data'][np.isfinite(g['data'])]).max())
        np.testing.assert_allclose(anomaly.values, want, rtol=0., atol=atol, equal_nan=True)
    me, anomaly = monthly_climo_error(da, g['val_set'], method='acc', n_fhour=2, return_da=True)
    assert isinstance(me, np.ndarray) and me.tolist() == [0., 0.] and anomaly.values.shape == g['anomaly_month_own'].shape
    with pytest.raises(AssertionError, match="'method' must be one of 'mse', 'mae', 'rmse', 'acc', 'cos'"):
        monthly_climo_error(da, g['val_set'], method='bias')
    with pytest.raises(KeyError, match='2004-07-04'):
        monthly_climo_error(da, np.concatenate([g['val_set'][:3], g['missing_time']]))
    early = g['times'][:4]                                                  # December 2003: not a month of the given climatology
    with pytest.raises(KeyError, match=r'\b12\b'):
        monthly_climo_error(da, early, climo_da=_climo_da(g, 'month'))
    with pytest.raises(ValueError, match='expected'):
        monthly_climo_error(da, g['val_set'], climo_da=_climo_da(g, 'dayofyear'))


@pytest.mark.parametrize('method', ['acc', 'cos'])
def test_lookup_through_the_host_forecast_error_equals_the_materialised_array_bitwise(g, method):
    from DLWP.verify import daily_climatology, daily_climo_time_series, forecast_error
    clim = daily_climatology(labelled(g['data'], g['times']))
    clim.values = np.nan_to_num(clim.values, nan=270., posinf=300.)
    ts, f_hour = g['ts_times'], g['ts_f_hour']
    rng = np.random.default_rng(3)
    shape = (len(f_hour), len(ts)) + g['data'].shape[1:]
    dims = ('f_hour',) + DIMS
    co = {'f_hour': f_hour, 'time': ts}
    co.update({d: np.arange(s) for d, s in zip(DIMS[1:], shape[2:])})
    fc = Forecast((rng.standard_normal(shape) * 3 + 280).astype(np.float32), dims, co)
    ver = Forecast((rng.standard_normal(shape) * 3 + 280).astype(np.float32), dims, co)
    ver.lat = Forecast(g['lat'], ['x0', 'x1', 'x2'], {d: co[d] for d in ('x0', 'x1', 'x2')})
    lazy = daily_climo_time_series(clim, ts, f_hour, lazy=True)
    full = daily_climo_time_series(clim, ts, f_hour)
    for kw in ({}, {'axis': (1, 2, 3, 4), 'weighted': True}):
        a = forecast_error(fc, ver, method, climatology=lazy, **kw)
        b = forecast_error(fc, ver, method, climatology=full, **kw)
        assert a.shape == b.shape and np.isfinite(a).all() and np.array_equal(a, b)


def test_estimator_climatology_on_a_host_generator(g):
    from DLWP.keras import backend
    from DLWP.model import DLWPFunctional, TimeSeriesEstimator
    from DLWP.model.generators import ArrayDataGenerator
    from DLWP.verify import daily_climatology
    prev = backend.device()
    backend.set_device('cpu')
    try:
        n = 120
        times = g['times'][:n]
        arr = np.ascontiguousarray(np.repeat(g['data'][:n], 2, axis=3).transpose(0, 4, 1, 2, 3))     # (T, V, 6, 2, 4)... square faces
        arr = np.ascontiguousarray(arr[..., :2, :2])
        dlwp = DLWPFunctional(is_convolutional=True, time_dim=2)

        class _Net(object):
            outputs = [None]

            def compile(self, **kw):
                pass
        dlwp.build_model(_Net(), loss='mse')
        gen = ArrayDataGenerator(dlwp, arr, rank=3, batch_size=4, input_time_steps=2, output_time_steps=2, channels_last=True)
        with pytest.raises(ValueError, match='no dates'):
            TimeSeriesEstimator(dlwp, gen).climatology()
        est = TimeSeriesEstimator(dlwp, gen, sample_times=times)
        cl = np.ascontiguousarray(arr.transpose(0, 2, 3, 4, 1))
        for by in ('dayofyear', 'month'):
            want = daily_climatology(labelled(cl, times), by=by)
            got = est.climatology(by=by)
            assert got.dims == (by, 'x0', 'x1', 'x2', 'varlev') and np.array_equal(got.coords[by], want.coords[by])
            assert isinstance(got.values, np.ndarray) and np.array_equal(got.values, want.values, equal_nan=True)
        rows = np.arange(10, 90, 3)
        want = daily_climatology(labelled(cl[rows], times[rows]))
        got = est.climatology(samples=rows)
        assert np.array_equal(got.coords['dayofyear'], want.coords['dayofyear'])
        assert np.array_equal(got.values, want.values, equal_nan=True)
    finally:
        backend.set_device(prev)
