#!/usr/bin/env python3
"""
Golden vectors for the climatology functions `daily_climatology`, `daily_climo_time_series` and `monthly_climo_error`
(reference DLWP/verify.py:167-214, 426-456).

The three reference bodies are xarray calls and xarray is not installed where this script runs, so they cannot be executed.
The expected values are an fp64 numpy restatement of the xarray calls those bodies make:
  * `ds.groupby('time.dayofyear' | 'time.month').mean()` (:187-188, :433): per element, np.nanmean over the rows of every
    present key, keys ascending;
  * `climatology.sel(dayofyear=doy)` (:450, :455): the row of the exact label, KeyError when it is absent;
  * `da.sel(time=val_set).groupby(...) - climo_da` (:189): every selected row minus the climatology row of its own key;
  * `(anomaly ** 2. * weights).mean()`, `(anomaly.abs() * weights).mean()` (:195-200): np.nanmean over everything, the
    weights cos(deg2rad(lat)) / mean (:190-192) broadcast by dimension name; 'acc' and 'cos' give 0. (:201-204).
Every calendar quantity -- day of the year, month, the roll-over of t + f hours (:449 `pd.Timestamp(t + np.array(f).astype(
'timedelta64[h]')).dayofyear`) -- comes from pandas, never from the code under test.  The script holds no reference program text.

Data: a 6-hourly series 2003-12-20 .. 2005-01-10 (a leap year, day 366, a year boundary) thinned so that days have 1, 4 and 8
members over the years, fp32 field (x0, x1, x2, varlev) = (6, 2, 2, 2) channels-last (tests transpose it for channels-first),
scattered NaNs, one (day, element) whose members are all NaN, one +inf.
Output: tests/golden/g15_climatology.npz.  Tests read the .npz only.
"""
import json
import os
import warnings

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
FIELD = (6, 2, 2, 2)
METHODS = ['mse', 'mae', 'rmse', 'acc', 'cos']


def series():
    rng = np.random.default_rng(15)
    full = pd.date_range('2003-12-20', '2005-01-10 18:00', freq='6h')
    keep = np.zeros(len(full), bool)
    for i, t in enumerate(full):
        every = (t.dayofyear % 7 == 0) or t.month in (12, 1) or (t.month == 2 and t.day >= 27) or (t.month == 3 and t.day <= 10)
        keep[i] = every or t.hour == 6
    times = full[keep]
    x = (rng.standard_normal((len(times),) + FIELD) * 3. + 280.).astype(np.float32)
    x[..., 1] = (rng.standard_normal((len(times),) + FIELD[:-1]) * 0.01).astype(np.float32)     # a variable that cancels
    nan_at = rng.random(x.shape) < 0.01
    x[nan_at] = np.nan
    day = np.asarray(times.normalize() == pd.Timestamp('2004-03-10'))
    assert day.sum() == 4
    x[day, 0, 0, 0, 0] = np.nan                                                                    # an all-NaN (day, element)
    at = int(np.nonzero(np.asarray(times == pd.Timestamp('2005-01-05 06:00')))[0][0])
    x[at, 3, 1, 0, 0] = np.inf
    return times, x


def nanmean(a, axis=None):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        with np.errstate(invalid='ignore'):
            return np.nanmean(a, axis=axis)


def group_mean(x, keys):
    """groupby(key).mean(): (present keys ascending, fp64 nanmean per key)"""
    uniq = np.unique(keys)
    return uniq.astype(np.int64), np.stack([nanmean(x[keys == k].astype(np.float64), axis=0) for k in uniq])


def lead_days(times, f_hour):
    """verify.py:449"""
    return np.array([[pd.Timestamp(t + np.array(f).astype('timedelta64[h]')).dayofyear for t in times] for f in f_hour],
                    dtype=np.int64)


def main():
    times, x = series()
    tv = times.values.astype('datetime64[h]')
    doy, month = np.asarray(times.dayofyear, np.int64), np.asarray(times.month, np.int64)
    members = np.bincount(doy)
    assert {1, 4, 8} <= set(members.tolist()) and 366 in doy and 60 in doy
    out = {'times': tv, 'data': x, 'doy': doy, 'month': month}
    out['doy_keys'], out['doy_mean'] = group_mean(x, doy)
    out['month_keys'], out['month_mean'] = group_mean(x, month)
    d0 = int(np.searchsorted(out['doy_keys'], pd.Timestamp('2004-03-10').dayofyear))
    assert np.isnan(out['doy_mean'][d0, 0, 0, 0, 0]) and members[out['doy_keys'][d0]] == 4
    assert np.isinf(out['doy_mean']).sum() == 1

    # calendar keys of every day of 1999-2004 (and a few hours inside the days)
    cal = pd.date_range('1999-01-01', '2004-12-31 23:00', freq='D') + pd.to_timedelta(np.arange(2192) % 24, unit='h')
    out['cal_times'] = cal.values.astype('datetime64[h]')
    out['cal_doy'], out['cal_month'] = np.asarray(cal.dayofyear, np.int64), np.asarray(cal.month, np.int64)

    # daily_climo_time_series: times around 31 December, 29 February and the year boundary; leads that cross them
    ts = pd.DatetimeIndex(['2003-12-31 18:00', '2004-02-27 12:00', '2004-02-28 18:00', '2004-02-29 06:00', '2004-03-01 00:00',
                           '2004-06-15 06:00', '2004-12-30 18:00', '2004-12-31 06:00', '2004-12-31 18:00', '2005-01-01 00:00'])
    f_hour = np.array([0, 6, 18, 24, 48, 72], dtype=np.int64)
    out['ts_times'] = ts.values.astype('datetime64[h]')
    out['ts_f_hour'] = f_hour
    out['ts_doy_none'] = np.asarray(ts.dayofyear, np.int64)
    out['ts_doy_lead'] = lead_days(ts.values, f_hour)
    assert {366, 1, 60, 61} <= set(out['ts_doy_lead'].reshape(-1).tolist())

    # monthly_climo_error: a strict subset of the times (February .. November 2004, every third row)
    pick = np.nonzero(np.asarray((times.year == 2004) & (times.month >= 2) & (times.month <= 11)))[0][::3]
    out['val_set'] = tv[pick]
    lat = np.linspace(-75., 80., int(np.prod(FIELD[:3]))).reshape(FIELD[:3])
    out['lat'] = lat
    w = np.cos(np.deg2rad(lat))
    w = (w / w.mean())[None, ..., None]
    rng = np.random.default_rng(16)
    given = {}
    for by, keys in (('month', month), ('dayofyear', doy)):
        k, m = group_mean(x + np.float32(0.5), keys)
        m = (m + 0.1 * rng.standard_normal(m.shape)).astype(np.float32)
        need = np.isin(k, np.unique(keys[pick]))
        given[by] = (k[need], m[need])
        out['given_%s_keys' % by], out['given_%s' % by] = given[by]
    cases = []
    for by_doy in (False, True):
        by, keys = ('dayofyear', doy) if by_doy else ('month', month)
        for have_climo in (False, True):
            if have_climo:
                ck, cm = given[by][0], given[by][1].astype(np.float64)
            else:
                ck, cm = group_mean(x, keys)
            anomaly = x[pick].astype(np.float64) - cm[np.searchsorted(ck, keys[pick])]
            tag = 'anomaly_%s_%s' % (by, 'given' if have_climo else 'own')
            out[tag] = anomaly.astype(np.float32)
            for weighted in (False, True):
                ww = w if weighted else 1.
                for method in METHODS:
                    if method == 'mse':
                        me = float(nanmean(anomaly ** 2. * ww))
                    elif method == 'mae':
                        me = float(nanmean(np.abs(anomaly) * ww))
                    elif method == 'rmse':
                        me = float(np.sqrt(nanmean(anomaly ** 2. * ww)))
                    else:
                        me = 0.
                    assert np.isfinite(me)
                    cases.append({'method': method, 'by_day_of_year': by_doy, 'weighted': weighted, 'climo_da': have_climo,
                                  'n_fhour': 3 if (weighted and method == 'rmse') else None, 'anomaly': tag, 'value': me})
    out['cases'] = json.dumps(cases)

    # KeyError cases: a time the data does not hold; a day the (partial) climatology does not hold
    out['missing_time'] = np.array(['2004-07-04T03'], dtype='datetime64[h]')
    assert out['missing_time'][0] not in tv
    part = given['dayofyear'][0]
    out['missing_day_times'] = np.array(['2004-06-15T06', '2004-01-02T00'], dtype='datetime64[h]')
    out['missing_day'] = np.int64(pd.Timestamp('2004-01-02').dayofyear)
    assert pd.Timestamp('2004-06-15').dayofyear in part and out['missing_day'] not in part
    np.savez_compressed(os.path.join(HERE, 'g15_climatology.npz'), **out)
    print('wrote g15_climatology.npz: %d rows, %d cases, %d bytes' % (len(times), len(cases),
                                                                     os.path.getsize(os.path.join(HERE, 'g15_climatology.npz'))))


if __name__ == '__main__':
    main()
