"""
Climatologies of DLWP.verify: grouped means and quantiles over the time axis, the series laid out from them, and the
month-aware climatology error.  The package docstring states the conventions.
"""
import numpy as np

from ..labelled import (coord, device_f32, device_scope, Forecast, host as _host, is_tensor as _is_tensor, label, labels,
                        on_device as _on_device, raw as _raw)
from .scores import _METHODS, _METHOD_MSG, _bstrides, _dev_operand, _score_host, _weights

# --------------------------------------------------------------------------------------------------------------------- #
# Climatologies (reference DLWP/verify.py:167-214 monthly_climo_error, :426-456 daily_climatology / daily_climo_time_series)
# --------------------------------------------------------------------------------------------------------------------- #

_BY = ('dayofyear', 'month')


def calendar_keys(times, by='dayofyear'):
    """int64 month (1..12) or day of the year (1 January = 1, so 29 February = 60 and 31 December of a leap year = 366) of
    every datetime64 in `times`: numpy datetime64 arithmetic only"""
    if by not in _BY:
        raise ValueError("'by' must be 'dayofyear' or 'month'")
    t = np.asarray(getattr(times, 'values', times))
    if t.dtype.kind != 'M':
        raise TypeError('the time coordinate must be datetime64, got %s' % t.dtype)
    if by == 'month':
        return t.astype('datetime64[M]').astype(np.int64) % 12 + 1
    day = t.astype('datetime64[D]')
    return (day - day.astype('datetime64[Y]').astype('datetime64[D]')).astype(np.int64) + 1


def _csr(keys):
    """(sorted present keys, group_start, row_index): rows grouped by key, in time order inside a group"""
    uniq, inv = np.unique(keys, return_inverse=True)
    order = np.argsort(inv.reshape(-1), kind='stable')
    start = np.concatenate([[0], np.cumsum(np.bincount(inv.reshape(-1), minlength=len(uniq)))])
    return uniq.astype(np.int64), start.astype(np.int64), order.astype(np.int64)


def _group_mean_host(v, axis, start, order, out_perm=None):
    """the formula of dlwpcs_group_mean in numpy: per element, the fp64 sum of the non-NaN members over their count, one
    rounding to fp32; an element with no member is NaN"""
    x = np.moveaxis(np.asarray(v), axis, 0)
    out = np.empty((len(start) - 1,) + x.shape[1:], dtype=np.float32)
    with np.errstate(invalid='ignore', divide='ignore'):
        for k in range(len(start) - 1):
            rows = np.asarray(x[order[start[k]:start[k + 1]]], dtype=np.float64)
            ok = ~np.isnan(rows)
            n = ok.sum(axis=0)
            out[k] = np.where(n > 0, np.where(ok, rows, 0.).sum(axis=0) / np.maximum(n, 1), np.nan)
    out = np.moveaxis(out, 0, axis)
    return out if out_perm is None else np.ascontiguousarray(out.transpose(out_perm))


def _climatology(ds, time_dim, by, rows=None, out_perm=None):
    """grouped mean of ds.values over `time_dim` (rows: restrict to these positions) -> (values, present keys)"""
    dims = tuple(ds.dims)
    if time_dim not in dims:
        raise ValueError("the data has no '%s' dimension (dims: %s)" % (time_dim, ', '.join(dims)))
    axis = dims.index(time_dim)
    times = coord(ds, time_dim)
    v = _raw(ds)
    if times.shape[0] != v.shape[axis]:
        raise ValueError("the '%s' coordinate has %d entries but its axis %d" % (time_dim, times.shape[0], v.shape[axis]))
    sel = np.arange(times.shape[0]) if rows is None else np.asarray(rows, dtype=np.int64).reshape(-1)
    uniq, start, order = _csr(calendar_keys(times[sel], by))
    order = sel[order]
    if _on_device(v):
        from .. import ops as dops
        with device_scope(v):
            return dops.group_mean(device_f32(v), start, order, row_axis=axis, out_perm=out_perm), uniq
    return _group_mean_host(_host(v), axis, start, order, out_perm), uniq


def daily_climatology(ds, *, by='dayofyear'):
    """
    Generate a daily climatology from labelled data with a 'time' dimension (reference DLWP/verify.py:426-433:
    `ds.groupby('time.dayofyear').mean()`): per element, the mean over the times of each day of the year, NaN skipped.

    :param ds: a `Forecast`, or anything with `.dims`, `.coords` and `.values`; 'time' (datetime64 coordinate) on any axis.
        Values on a HIP device are reduced there (dlwpcs_group_mean) and the result stays there; numpy values are reduced on the
        host in fp64.
    :param by: 'dayofyear' or 'month' (the grouping `monthly_climo_error` uses)
    :return: Forecast, fp32, with the 'time' dimension replaced by `by`; its coordinate holds the sorted present keys (int64)
    """
    values, uniq = _climatology(ds, 'time', by)
    return label(ds, values, 'climatology', replace={tuple(ds.dims).index('time'): (by, uniq)}, lat=True)


def _group_quantile_host(v, axis, start, order, probs, out_perm=None):
    """the formula of dlwpcs_group_quantile in numpy: per element the non-NaN members sorted, h = (n - 1) p, j = floor(h),
    g = h - j, x_(j) + g (x_(j+1) - x_(j)) in fp64 (x_(j) itself where g = 0), one rounding to fp32; -0 enters as +0, an
    element with no member is NaN.  The probabilities lead."""
    x = np.moveaxis(np.asarray(v), axis, 0)
    p = np.asarray(probs, dtype=np.float64).reshape((-1,) + (1,) * (x.ndim - 1))
    out = np.empty((p.shape[0], len(start) - 1) + x.shape[1:], dtype=np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        for k in range(len(start) - 1):
            rows = np.sort(np.asarray(x[order[start[k]:start[k + 1]]], dtype=np.float64) + 0.0, axis=0)     # NaN sorts last
            if rows.shape[0] == 0:
                out[:, k] = np.nan
                continue
            n = (~np.isnan(rows)).sum(axis=0)
            h = np.maximum(n - 1, 0)[None] * p
            j = np.floor(h)
            g = h - j
            lo = j.astype(np.int64)
            hi = np.minimum(lo + 1, rows.shape[0] - 1)
            xj, xj1 = np.take_along_axis(rows[None], lo[:, None], axis=1)[:, 0], np.take_along_axis(rows[None], hi[:, None], axis=1)[:, 0]
            val = np.where(g == 0, xj, xj + g * (xj1 - xj))
            out[:, k] = np.where((n[None] > 0) & ~np.isnan(val), val, np.nan)       # (inf - inf: the same quiet NaN)
    out = np.moveaxis(out, 1, axis + 1)
    return out if out_perm is None else np.ascontiguousarray(out.transpose((0,) + tuple(a + 1 for a in out_perm)))


def climatology_quantiles(ds, q, *, by='dayofyear'):
    """
    Climatological quantiles of labelled data with a 'time' dimension: per element and per group of times, numpy's default
    ('linear') quantiles of the values that are not NaN -- the tercile boundaries the categorical scores (`categorical_error`)
    are computed against.

    :param ds: a `Forecast`, or anything with `.dims`, `.coords` and `.values`; 'time' (datetime64 coordinate) on any axis.
        Values on a HIP device are reduced there (dlwpcs_group_quantile) and the result stays there; numpy values are reduced on
        the host in fp64.  Both interpolate in fp64 and round to fp32 once.
    :param q: up to 16 probabilities in [0, 1] (a scalar counts as one), e.g. (1 / 3, 2 / 3)
    :param by: 'dayofyear', 'month', or None: all times in one group
    :return: Forecast, fp32, dims ('quantile',) + the dims of `ds` with 'time' replaced by `by` (by=None: without it); the
        'quantile' coordinate is `q`, the `by` coordinate holds the sorted present keys (int64).  NaN where a group has no
        value.  A table by 'dayofyear' is what `daily_climo_time_series` lays out along forecast times.
    """
    p = np.atleast_1d(np.asarray(q, dtype=np.float64)).reshape(-1)
    if not 1 <= p.size <= 16:
        raise ValueError('climatology_quantiles: %d probabilities (1 .. 16)' % p.size)
    if not np.all((p >= 0.) & (p <= 1.)):
        raise ValueError('climatology_quantiles: probabilities must lie in [0, 1], got %s' % (p,))
    if by is not None and by not in _BY:
        raise ValueError("'by' must be 'dayofyear', 'month' or None")
    dims = tuple(ds.dims)
    if 'time' not in dims:
        raise ValueError("the data has no 'time' dimension (dims: %s)" % ', '.join(dims))
    axis = dims.index('time')
    v = _raw(ds)
    if by is None:
        nt = int(v.shape[axis])
        uniq, start, order = np.zeros(1, dtype=np.int64), np.array([0, nt], dtype=np.int64), np.arange(nt, dtype=np.int64)
    else:
        times = coord(ds, 'time')
        if times.shape[0] != v.shape[axis]:
            raise ValueError("the 'time' coordinate has %d entries but its axis %d" % (times.shape[0], v.shape[axis]))
        uniq, start, order = _csr(calendar_keys(times, by))
    if _on_device(v):
        from .. import ops as dops
        with device_scope(v):
            values = dops.group_quantile(device_f32(v), start, order, p, row_axis=axis)
    else:
        values = _group_quantile_host(_host(v), axis, start, order, p)
    lead = [('quantile', p)]
    if by is None:
        return label(ds, values.squeeze(axis + 1), 'climatology_quantiles', drop=(axis,), lead=lead, lat=True)
    return label(ds, values, 'climatology_quantiles', replace={axis: (by, uniq)}, lead=lead, lat=True)


def _lead_hours(f_hour):
    """timedelta64[h] of every forecast hour: the reference's np.array(f).astype('timedelta64[h]') (:449), floats truncated"""
    f = np.asarray(getattr(f_hour, 'values', f_hour))
    if f.dtype.kind == 'f':
        f = np.trunc(f).astype(np.int64)
    return f.astype('timedelta64[h]')


class ClimatologyLookup(object):
    """
    A climatology time series that is not laid out: the (K, ...) climatology `table`, and for every (forecast hour,) time the
    row of the table that stands there (`rows`, int32).  It has the dims, coords and shape of the series it stands for;
    `materialize()` builds that series.  `forecast_error` takes it as `climatology` and looks the rows up inside the score.
    """

    def __init__(self, table, row_axis, rows, dims, coords, name='climatology'):
        self.table = table
        self.row_axis = int(row_axis)
        self.rows = np.ascontiguousarray(rows, dtype=np.int32)
        self.dims = tuple(dims)
        self.coords = dict(coords)
        self.name = name
        self._rows_dev = None

    @property
    def shape(self):
        t = tuple(int(s) for s in _raw(self.table).shape)
        series = t[:self.row_axis] + (self.rows.shape[-1],) + t[self.row_axis + 1:]
        return (self.rows.shape[0],) + series if self.rows.ndim == 2 else series

    def rows_on(self, dev):
        """the row table as an int32 device tensor (uploaded once)"""
        if self._rows_dev is None or self._rows_dev.device != dev:
            import torch
            self._rows_dev = torch.from_numpy(self.rows.reshape(-1)).pin_memory().to(dev, non_blocking=True)
        return self._rows_dev

    def materialize(self):
        """the series itself: a Forecast of `shape` (device values: one dlwpcs_rows_gather launch)"""
        t = _raw(self.table)
        ax, lead = self.row_axis, self.rows.ndim == 2
        split = tuple(t.shape[:ax]) + tuple(self.rows.shape) + tuple(t.shape[ax + 1:])
        if _on_device(t):
            from .. import ops as dops
            with device_scope(t) as dev:
                v = dops.rows_gather(device_f32(t), self.rows_on(dev), row_axis=ax).reshape(split)
            v = v.movedim(ax, 0) if lead else v
        else:
            v = np.take(np.asarray(_host(t), dtype=np.float32), self.rows.reshape(-1), axis=ax).reshape(split)
            v = np.moveaxis(v, ax, 0) if lead else v
        return Forecast(v, self.dims, self.coords, name=self.name)


def daily_climo_time_series(climatology, times, f_hour=None, *, lazy=False):
    """
    Generate a time series of daily climatology values from a climatology and the desired times (reference
    DLWP/verify.py:436-456): the value at (f, t) is the climatology of the day of the year of t + f hours.

    :param climatology: labelled climatology with a 'dayofyear' dimension (`daily_climatology`)
    :param times: datetime64 times
    :param f_hour: None, or forecast hours as ints / floats / timedelta64
    :param lazy: True returns a `ClimatologyLookup` instead of the series (nothing of the series' size is allocated)
    :return: Forecast with the 'dayofyear' dimension replaced by 'time' (behind a leading 'f_hour' when given), coordinates
        `times` / `f_hour`.  A day the climatology does not hold raises KeyError naming it.
    """
    dims = tuple(climatology.dims)
    if 'dayofyear' not in dims:
        raise ValueError("the climatology has no 'dayofyear' dimension (dims: %s)" % ', '.join(dims))
    axis = dims.index('dayofyear')
    have = coord(climatology, 'dayofyear').astype(np.int64)
    t = np.asarray(getattr(times, 'values', times))
    if t.dtype.kind != 'M':
        t = t.astype('datetime64[ns]')
    if f_hour is None:
        when = t
    else:
        when = t.astype('datetime64[s]')[None, :] + _lead_hours(f_hour).astype('timedelta64[s]')[:, None]
    doy = calendar_keys(when, 'dayofyear')
    rows = _sel_rows(have, doy, 'dayofyear')
    lead = () if f_hour is None else [('f_hour', getattr(f_hour, 'values', f_hour))]
    look = ClimatologyLookup(_raw(climatology), axis, rows, *labels(climatology, replace={axis: ('time', t)}, lead=lead))
    return look if lazy else look.materialize()


def _sel_rows(labels, wanted, what):
    """position of every wanted label in `labels` (exact match, as .sel); KeyError names the first that is missing"""
    order = np.argsort(labels, kind='stable')
    srt = labels[order]
    flat = np.asarray(wanted).reshape(-1)
    if len(srt) == 0:
        if flat.size:
            raise KeyError('%s %s is not in the data' % (what, flat[0]))
        return np.zeros(np.shape(wanted), dtype=np.int32)
    pos = np.minimum(np.searchsorted(srt, flat), len(srt) - 1)
    miss = srt[pos] != flat
    if miss.any():
        raise KeyError('%s %s is not in the data' % (what, flat[np.argmax(miss)]))
    return order[pos].astype(np.int32).reshape(np.shape(wanted))


def monthly_climo_error(da, val_set, n_fhour=None, method='mse', climo_da=None, by_day_of_year=False, return_da=False,
                        weighted=False):
    """
    Calculates a month-aware climatology error for a validation set (reference DLWP/verify.py:167-214).

    :param da: labelled data with a 'time' or 'sample' dimension ('sample' is preferred) with a datetime64 coordinate
    :param val_set: times for which to calculate an error; each must be a time of `da` (KeyError otherwise)
    :param n_fhour: int or None: if int, the error is repeated into an array of length n_fhour
    :param method: 'mse', 'mae', 'rmse'; 'acc' and 'cos' return zeros
    :param climo_da: pre-computed monthly or daily climatology (dimension 'month' / 'dayofyear' in place of the time dimension)
    :param by_day_of_year: climatology by day of year instead of monthly
    :param return_da: also return the anomaly (a Forecast with the dims of `da`, its time dimension = val_set)
    :param weighted: weight by cos(latitude) read from `da.lat`
    :return: float or ndarray[, Forecast].  Device values are scored by one dlwpcs_score_indexed call.
    """
    assert method in _METHODS, _METHOD_MSG
    dims = tuple(da.dims)
    time_dim = 'sample' if 'sample' in dims else 'time'
    parameter = 'dayofyear' if by_day_of_year else 'month'
    if time_dim not in dims:
        raise ValueError("the data has no 'sample' or 'time' dimension (dims: %s)" % ', '.join(dims))
    axis = dims.index(time_dim)
    times = coord(da, time_dim)
    if climo_da is None:
        table, keys = _climatology(da, time_dim, parameter)
    else:
        want = tuple(parameter if d == time_dim else d for d in dims)
        if tuple(climo_da.dims) != want:
            raise ValueError('the climatology has dims %s, expected %s' % (tuple(climo_da.dims), want))
        table, keys = _raw(climo_da), coord(climo_da, parameter).astype(np.int64)
    wanted = np.asarray(getattr(val_set, 'values', val_set)).reshape(-1)
    if wanted.dtype.kind != 'M':
        wanted = wanted.astype(times.dtype)
    sel = _sel_rows(times, wanted.astype(times.dtype), time_dim).astype(np.int64)
    rows = _sel_rows(keys, calendar_keys(times[sel], parameter), parameter)
    w = _weights(da) if weighted else None
    if w is not None and np.ndim(w) == len(dims):
        w = np.moveaxis(w, axis, 0)                        # beside the time-first views below
    device = _on_device(da, table)
    anomaly = None
    if method in ('acc', 'cos') and not return_da:
        me = 0.
    elif device:
        me, anomaly = _climo_error_device(method, _raw(da), table, axis, sel, rows, w, return_da)
    else:
        x = np.asarray(np.moveaxis(_host(da), axis, 0)[sel], dtype=np.float64)
        anomaly = x - np.asarray(np.moveaxis(_host(table), axis, 0)[rows], dtype=np.float64)
        wh = 1. if w is None else w
        me = 0. if method in ('acc', 'cos') else float(_score_host(method, 0., anomaly, 0., wh, None))
        anomaly = np.moveaxis(anomaly.astype(np.float32), 0, axis)
    if method == 'rmse':
        me = np.sqrt(me) if device else np.float64(me)
    if n_fhour is not None:
        me = np.array([me] * n_fhour)
    if return_da:
        return me, label(da, anomaly, 'anomaly', select={axis: sel})
    return me


def _climo_error_device(method, v, table, axis, sel, rows, w, want_anomaly):
    """the score of v's rows `sel` (time axis `axis`) against the table rows `rows`, on the device: (float, anomaly or None)"""
    import torch
    from .. import ops as dops
    dev = next(x.device for x in (v, table) if _is_tensor(x) and x.is_cuda)
    with torch.cuda.device(dev):
        vt, tt = _dev_operand(v, dev).movedim(axis, 0), _dev_operand(table, dev).movedim(axis, 0)
        step = int(sel[1] - sel[0]) if len(sel) > 1 else 1
        if len(sel) and step > 0 and np.array_equal(sel, sel[0] + step * np.arange(len(sel))):
            b = vt[int(sel[0]):int(sel[-1]) + 1:step]         # a view: the selected rows are evenly spaced
        else:
            b = dops.rows_gather(vt, sel, row_axis=0)
        anomaly = None
        if want_anomaly:
            anomaly = (b - dops.rows_gather(tt, rows, row_axis=0)).movedim(0, axis)
        if method in ('acc', 'cos'):
            return 0., anomaly
        n = int(b.shape[0])
        shape = (1, n) + tuple(int(s) for s in b.shape[1:])
        ops_ = [(tt, (0, 0) + tuple(int(s) for s in tt.stride()[1:])), (b, (0,) + tuple(int(s) for s in b.stride())), None]
        if w is not None:
            wt = _dev_operand(w, dev)
            ws = wt.reshape(tuple(wt.shape[1:])) if wt.dim() == b.dim() and wt.shape[0] == 1 else wt
            if ws.dim() >= b.dim():
                raise ValueError('the weights of %s do not broadcast against the data behind its time axis' % (tuple(wt.shape),))
            ops_.append((ws, (0, 0) + _bstrides(ws, shape[2:])))
        else:
            ops_.append(None)
        idx = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).pin_memory().to(dev, non_blocking=True)
        kind = 'mse' if method == 'rmse' else method            # the reference takes the root of a Python float (:203)
        out = dops.score_reduce(kind, ops_, shape, set(range(1, len(shape))), lagged=(n, 0),
                                indexed=(idx, int(tt.stride(0))))
        return float(out.cpu().numpy().reshape(-1)[0]), anomaly
