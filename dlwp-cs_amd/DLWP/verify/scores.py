"""
Forecast scores of DLWP.verify: `forecast_error`, `persistence_error`, `climo_error`, the labelling of a cubed-sphere forecast
(`add_metadata_to_forecast_cs`), and what the other families take from here: the latitude weights, the host restatement of
the score formulas and the device operands of the score reduction.  The package docstring states the conventions.
"""
import warnings

import numpy as np

from ..labelled import axes as _axes, coord, device_scope, Forecast, host as _host, on_device as _on_device, raw as _raw

_SPATIAL = ('face', 'height', 'width')


def _data_dims(split_levels, channels_last):
    """Names of the axes behind `f_hour`, in storage order; the sample axis is labelled 'time' in the result."""
    channel = ('variable', 'level') if split_levels else ('varlev',)
    return ('sample',) + (_SPATIAL + channel if channels_last else channel + _SPATIAL)


def add_metadata_to_forecast_cs(forecast, f_hour, meta_ds, f_hour_timedelta_type=False, channels_last=False):
    """
    Label `forecast` (forecast hour, initialisation time, then channels and the face / height / width axes in the order
    `channels_last` says) with the coordinates of `meta_ds`.

    When `meta_ds` has a 'level' dimension the single channel axis is unfolded into ('variable', 'level') with the sizes
    `meta_ds.dims` gives; otherwise it is 'varlev'.  `f_hour_timedelta_type` turns the forecast-hour coordinate into
    numpy timedelta64[h].  Raises ValueError when `f_hour` and the first axis disagree, or a coordinate does not fit its axis.
    """
    values = np.asarray(getattr(forecast, 'values', forecast))
    lead = np.asarray(f_hour)
    if lead.shape[0] != values.shape[0]:
        raise ValueError("'f_hour' coordinate must have same size as the first axis of 'forecast'")
    if f_hour_timedelta_type:
        lead = lead.astype('timedelta64[h]')
    split = 'level' in meta_ds.dims
    source = _data_dims(split, channels_last)
    if split:
        values = values.reshape((lead.shape[0],) + tuple(int(meta_ds.dims[d]) for d in source))
    names = ('f_hour',) + tuple('time' if d == 'sample' else d for d in source)
    coords = {'f_hour': lead}
    for name, src in zip(names[1:], source):
        c = meta_ds[src]
        coords[name] = np.asarray(getattr(c, 'values', c))
    if values.ndim != len(names):
        raise ValueError('forecast has %d axes, expected %d: %s' % (values.ndim, len(names), ', '.join(names)))
    for axis, name in enumerate(names):
        if coords[name].shape[0] != values.shape[axis]:
            raise ValueError('axis %d (%s) has %d entries but its coordinate has %d'
                             % (axis, name, values.shape[axis], coords[name].shape[0]))
    return Forecast(values, list(names), coords, name='forecast')


# --------------------------------------------------------------------------------------------------------------------- #
# Scores
# --------------------------------------------------------------------------------------------------------------------- #

_METHODS = ['mse', 'mae', 'rmse', 'acc', 'cos']
_METHOD_MSG = "'method' must be one of 'mse', 'mae', 'rmse', 'acc', 'cos'"


def _check_labels(forecast, valid):
    """labelled inputs must agree on dims and coordinates (a continuous series: on the axes behind the time axis): xarray's
    inner join is not reproduced"""
    if not (hasattr(forecast, 'dims') and hasattr(valid, 'dims')):
        return
    fd, vd = tuple(forecast.dims), tuple(valid.dims)
    lagged = len(vd) == len(fd) - 1
    if (fd[2:] != vd[1:]) if lagged else (fd != vd):
        raise ValueError('forecast dims %s do not match the verification dims %s' % (fd, vd))
    fc, vc = getattr(forecast, 'coords', {}), getattr(valid, 'coords', {})
    for d in (fd[2:] if lagged else fd):
        if d in fc and d in vc:
            a, b = coord(forecast, d), coord(valid, d)
            if a.shape != b.shape or not np.array_equal(a, b):
                raise ValueError("coordinate '%s' of the forecast and the verification differ (no alignment is done)" % d)


def _weights(valid):
    """cos(deg2rad(valid.lat)) / its mean, shaped to broadcast against `valid`: by dimension name when both carry `.dims`
    (xarray's rule), else as it is (numpy's trailing-axis rule)"""
    lat = valid.lat
    w = np.cos(np.deg2rad(np.asarray(_host(lat), dtype=np.float64)))
    w = w / w.mean()
    if hasattr(valid, 'dims') and hasattr(lat, 'dims'):
        ld = tuple(lat.dims)
        missing = [d for d in ld if d not in valid.dims]
        if missing:
            raise ValueError('lat has dims %s that the verification lacks' % missing)
        order = [ld.index(d) for d in valid.dims if d in ld]
        w = np.transpose(w, order).reshape([w.shape[ld.index(d)] if d in ld else 1 for d in valid.dims])
    return w


# ---- host path: numpy restatement --------------------------------------------------------------------------------- #

def _nanmean(x, axis):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        return np.nanmean(x, axis=axis)


def _cos_host(f, v, c, w, axis):
    ax = axis
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.sum((f - c) * ((v - c) * w), axis=ax) / (np.sqrt(np.sum(((f - c) * w) ** 2., axis=ax)) *
                                                           np.sqrt(np.sum(((v - c) * w) ** 2., axis=ax)))


def _score_host(method, f, v, c, w, axis):
    with np.errstate(invalid='ignore', divide='ignore'):
        if method == 'mse':
            return _nanmean((v - f) ** 2. * w, axis)
        if method == 'mae':
            return _nanmean(np.abs((v - f) * w), axis)
        if method == 'rmse':
            return np.sqrt(_nanmean((v - f) ** 2. * w, axis))
        if method == 'acc':
            return (_nanmean((v - c) * (f - c) * w, axis) /
                    np.sqrt(_nanmean((v - c) ** 2. * w, axis) * _nanmean((f - c) ** 2. * w, axis)))
        return _cos_host(f, v, c, w, axis)


# ---- device path: dlwpcs_score ------------------------------------------------------------------------------------ #

def _dev_operand(x, dev):
    """fp32 device tensor of x (a device tensor stays where it is; host data is uploaded through pinned memory)"""
    import torch
    r = _raw(x)
    if isinstance(r, torch.Tensor):
        return r if (r.device == dev and r.dtype == torch.float32) else r.to(dev, torch.float32)
    a = torch.from_numpy(np.ascontiguousarray(np.asarray(r, dtype=np.float32)).reshape(np.shape(r)))
    return a.pin_memory().to(dev, non_blocking=True)


def _bstrides(t, shape):
    """strides (elements) of tensor t broadcast to `shape` by numpy's trailing-axis rule (0 where broadcast)"""
    nd, td = len(shape), t.dim()
    if td > nd:
        raise ValueError('operands could not be broadcast together: %s and %s' % (tuple(t.shape), tuple(shape)))
    st = [0] * (nd - td)
    for i in range(td):
        e = int(t.shape[i])
        if e != 1 and e != shape[nd - td + i]:
            raise ValueError('operands could not be broadcast together: %s and %s' % (tuple(t.shape), tuple(shape)))
        st.append(int(t.stride(i)) if e != 1 else 0)
    return tuple(st)


def _const_operand(c, dev):
    """None for a zero / absent climatology, else (tensor, broadcast marker)"""
    if c is None:
        return None
    r = _raw(c)
    if np.ndim(r) == 0 and not hasattr(r, 'is_cuda'):
        if float(r) == 0.0:
            return None
    return _dev_operand(c, dev)


def _bshape(*shapes):
    return tuple(int(s) for s in np.broadcast_shapes(*[tuple(s) for s in shapes]))


def _aligned_device(method, f, v, c, w, axis):
    dev = (f if f.is_cuda else v).device
    shapes = [f.shape, v.shape] + [x.shape for x in (c, w) if x is not None]
    shape = _bshape(*shapes)
    nd = len(shape)
    red = set(range(nd)) if axis is None else set(axis)
    ops = [(x, _bstrides(x, shape)) if x is not None else None for x in (f, v, c, w)]
    from .. import ops as dops
    out = dops.score_reduce(method, ops, shape, red)
    return out.cpu().numpy()


def _lookup_serves(lookup, forecast, valid, method, axis):
    """whether dlwpcs_score_indexed can score this call: device operands with a forecast hour axis each, the table's rows on
    its first axis, the time axis reduced and the forecast hour kept, rows of a multiple of 4 elements"""
    if method not in ('acc', 'cos') or len(forecast.shape) != len(valid.shape) or len(forecast.shape) < 2:
        return False
    if not _on_device(forecast, valid, lookup.table) or lookup.row_axis != 0:
        return False
    nd = len(valid.shape)
    ax = tuple(range(1, nd)) if axis is None else _axes(axis, nd)
    if 0 in ax or 1 not in ax:
        return False
    if int(np.prod(forecast.shape[2:])) % 4 != 0:
        # a row of odd length: the array path may merge the time axis into 16-byte chunks that straddle rows, which a lookup
        # per row cannot follow in the same order -- materialise, so that the bits are those of the array path
        return False
    return lookup.rows.shape[-1] == forecast.shape[1] and (lookup.rows.ndim == 1 or lookup.rows.shape[0] == forecast.shape[0])


def _indexed_device(method, f, v, lookup, w, axis):
    """_aligned_device with the climatology looked up by row: the lagged form of the kernel with every time taking part"""
    import torch
    dev = (f if f.is_cuda else v).device
    table = _dev_operand(lookup.table, dev)
    n_lead, n_time = int(f.shape[0]), int(f.shape[1])
    series = (n_lead, n_time) + tuple(table.shape[1:])
    shape = _bshape(*([f.shape, v.shape, series] + ([w.shape] if w is not None else [])))
    if shape[:2] != (n_lead, n_time):
        raise ValueError('operands could not be broadcast together: %s and %s' % (tuple(f.shape), tuple(v.shape)))
    if lookup.rows.ndim == 2:
        rows = lookup.rows_on(dev)
    else:
        rows = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(lookup.rows, (n_lead, n_time))).reshape(-1)
                                ).pin_memory().to(dev, non_blocking=True)
    ops = [(f, _bstrides(f, shape)), (v, _bstrides(v, shape)), (table, (0, 0) + _bstrides(table[0], shape[2:])),
           (w, _bstrides(w, shape)) if w is not None else None]
    from .. import ops as dops
    out = dops.score_reduce(method, ops, shape, set(axis), lagged=(n_time, 0), indexed=(rows, int(table.stride(0))))
    return out.cpu().numpy()


def _lagged_device(method, a, a_lead, b, c, w, axis, n_lead, t_cap):
    """out[f] = score of a-rows [f*a_lead, ...) against b rows [f, f + n_f) with n_f = min(rows of a, t_cap - f), reduced
    over `axis` of the per-lead (n_f, S...) arrays.  a: (n_lead?, T, S...) when a_lead else (T, S...); b: (V, S...)."""
    import torch
    dev = b.device
    a_t = a if a_lead else a.unsqueeze(0).expand((n_lead,) + tuple(a.shape))
    if a_lead and a_t.shape[0] < n_lead:
        raise ValueError('forecast has %d leads, expected %d' % (a_t.shape[0], n_lead))
    T = int(a_t.shape[1])
    nd = b.dim()                                           # per-lead arrays are (n_f, S...)
    space = _bshape(tuple(a_t.shape[2:]), tuple(b.shape[1:]), *[tuple(x.shape[1:]) if x.dim() >= nd else tuple(x.shape)
                                                              for x in (c, w) if x is not None])
    if T < t_cap:
        raise ValueError('operands could not be broadcast together: the forecast has %d times, the verification %d'
                         % (T, t_cap))
    if n_lead - 1 > t_cap:
        raise ValueError('forecast hour %d lies past the end of the %d verification times' % (n_lead - 1, t_cap))
    shape = (n_lead, T) + space
    sa = _bstrides(a_t, shape)
    b_rows = _bstrides(b, (t_cap,) + space)               # the series has t_cap rows; only n_f <= t_cap - f are read
    sb = (b_rows[0],) + b_rows
    ops = [(a_t, sa), (b, sb)]
    for x in (c, w):
        if x is None:
            ops.append(None)
            continue
        xs = x.reshape(tuple(x.shape[1:])) if x.dim() >= nd and x.shape[0] == 1 else x
        if xs.dim() >= nd:
            raise ValueError('operands could not be broadcast together: %s against (%d, %s)' % (tuple(x.shape), T, space))
        st = _bstrides(xs, shape[2:])
        ops.append((xs, (0, 0) + st))
    red = {1} | (set(range(2, 2 + len(space))) if axis is None else set(a + 1 for a in axis if a > 0))
    from .. import ops as dops
    with torch.cuda.device(dev):
        out = dops.score_reduce(method, ops, shape, red, lagged=(t_cap, 1))
    return out.cpu().numpy()


# ---- public functions ------------------------------------------------------------------------------------------- #

def forecast_error(forecast, valid, method='mse', axis=None, weighted=False, climatology=None):
    """
    Calculate the error of a time series model forecast (reference DLWP/verify.py:18-97).

    :param forecast: forecast (forecast hour first): ndarray, device tensor or Forecast
    :param valid: verification with a forecast hour axis (same shape) or a continuous series (one axis fewer)
    :param method: 'mse', 'mae', 'rmse', 'acc' (anomaly correlation) or 'cos' (cosine similarity; labelled inputs)
    :param axis: int, tuple or None: axes to average over (None: every axis but the forecast hour)
    :param weighted: weight by cos(latitude) read from `valid.lat`
    :param climatology: climatology for 'acc' / 'cos': a number, an array, or a `ClimatologyLookup`
        (`daily_climo_time_series(..., lazy=True)`), whose rows are looked up inside the score on the device
    :return: float64 ndarray with forecast hour as the first dimension
    """
    assert method in _METHODS, _METHOD_MSG
    if method in ['acc', 'cos'] and climatology is None:
        warnings.warn("'acc' and 'cos' error methods expect to get a climatology; using 0 instead, which may yield "
                      "unexpected results.")
        climatology = 0.
    from .climatology import ClimatologyLookup      # upwards, so at call time: climatology builds on this module
    lookup = None
    if isinstance(climatology, ClimatologyLookup):
        if _lookup_serves(climatology, forecast, valid, method, axis):
            lookup, climatology = climatology, climatology.table
        else:                                              # the host path, and axes the indexed kernel does not serve
            climatology = climatology.materialize()
    _check_labels(forecast, valid)
    n_f = forecast.shape[0]
    w = _weights(valid) if weighted else None
    device = _on_device(forecast, valid, climatology)
    aligned = len(forecast.shape) == len(valid.shape)
    nd = len(valid.shape)
    if method == 'cos' and not hasattr(forecast, 'dims'):
        raise TypeError("'cos' method requires xarray DataArrays for now")
    if aligned:
        ax = tuple(range(1, nd)) if axis is None else _axes(axis, nd)
        if not device:
            f, v = _host(forecast), _host(valid)
            c = _host(climatology) if climatology is not None else 0.
            return np.asarray(_score_host(method, f, v, c, 1. if w is None else w, ax), dtype=np.float64)
        with device_scope(forecast, valid, climatology) as dev:
            f, v = _dev_operand(forecast, dev), _dev_operand(valid, dev)
            c = _const_operand(climatology, dev) if method in ('acc', 'cos') else None
            wt = _dev_operand(w, dev) if w is not None else None
            if lookup is not None:
                return np.asarray(_indexed_device(method, f, v, lookup, wt, ax), dtype=np.float64)
            return np.asarray(_aligned_device(method, f, v, c, wt, ax), dtype=np.float64)
    # valid given as a continuous time series without a forecast hour dimension
    clim_shape = np.shape(_raw(climatology)) if climatology is not None else ()
    if climatology is not None and np.ndim(_raw(climatology)) > 0 and len(clim_shape) >= nd and clim_shape[0] > 1:
        raise ValueError("'climatology' cannot have non-spatial dimensions != 1 if the verification data is not "
                         "provided with a forecast hour dimension")
    if method == 'cos':
        raise NotImplementedError("'cos' against a continuous verification series: the reference's dot(dims=axis) with "
                                  "integer axes (DLWP/verify.py:91-94) cannot run")
    n_val = valid.shape[0]
    ax = None if axis is None else _axes(axis, nd)
    if method == 'acc':
        # the reference returns from inside its loop: the f = 0 value only, without the weights (verify.py:87-90)
        if not device:
            f0, v = _host(forecast)[0, :n_val], _host(valid)
            c = _host(climatology)
            return np.asarray(_score_host('acc', f0, v, c, 1., ax), dtype=np.float64)
        with device_scope(forecast, valid, climatology) as dev:
            f0 = _dev_operand(forecast, dev)[0:1, :n_val]
            v = _dev_operand(valid, dev).unsqueeze(0)
            c = _const_operand(climatology, dev)
            full = tuple(a + 1 for a in ax) if ax is not None else tuple(range(1, nd + 1))
            return np.asarray(_aligned_device('acc', f0, v, c, None, full), dtype=np.float64)[0]
    if not device:
        f, v = _host(forecast), _host(valid)
        wh = 1. if w is None else w
        return np.array([_score_host(method, f[k, :(n_val - k)], v[k:], 0., wh, ax) for k in range(n_f)], dtype=np.float64)
    return _lagged_dispatch(method, forecast, True, valid, w, ax, n_f, n_val)


def _lagged_dispatch(method, a, a_lead, valid, w, ax, n_lead, n_val):
    with device_scope(a, valid) as dev:
        at, v = _dev_operand(a, dev), _dev_operand(valid, dev)
        wt = _dev_operand(w, dev) if w is not None else None
        if ax is not None and 0 not in ax:
            if n_lead > 1:
                raise ValueError('the per-lead results have different shapes (the time axis is kept): cannot be stacked')
            a0 = (at[0:1] if a_lead else at.unsqueeze(0))[:, :n_val]
            return np.asarray(_aligned_device(method, a0, v.unsqueeze(0), None, wt, tuple(x + 1 for x in ax)), dtype=np.float64)
        return np.asarray(_lagged_device(method, at, a_lead, v, None, wt, ax, n_lead, n_val), dtype=np.float64)


def persistence_error(predictors, valid, n_fhour, method='mse', axis=None, weighted=False):
    """
    Calculate the error of a persistence forecast out to n_fhour forecast hours (reference DLWP/verify.py:100-132).
    DEPRECATED in the reference as of version 0.8.4: use forecast_error with an array of persistence forecasts.

    :return: float64 ndarray with forecast hour as the first dimension
    """
    warnings.warn("'persistence_error' is deprecated as of version 0.8.4. Use 'forecast_error' with an "
                  "appropriate array of persistence forecasts instead.", DeprecationWarning)
    if method not in ['mse', 'mae', 'rmse']:
        raise ValueError("'method' must be 'mse', 'rmse', or 'mae'")
    n_f = valid.shape[0]
    w = _weights(valid) if weighted else None
    ax = None if axis is None else _axes(axis, len(valid.shape))
    if not _on_device(predictors, valid):
        p, v = _host(predictors), _host(valid)
        wh = 1. if w is None else w
        return np.array([_score_host(method, p[:(n_f - f)], v[f:], 0., wh, ax) for f in range(int(n_fhour))],
                        dtype=np.float64)
    return _lagged_dispatch(method, predictors, False, valid, w, ax, int(n_fhour), n_f)


def climo_error(valid, n_fhour, method='mse', axis=None, weighted=False):
    """
    Calculate the error of a climatology forecast out to n_fhour forecast hours (reference DLWP/verify.py:135-163): the
    first n - f verification times against nanmean(valid, axis=0).

    :return: float64 ndarray with forecast hour as the first dimension
    """
    if method not in ['mse', 'mae', 'rmse']:
        raise ValueError("'method' must be 'mse', 'rmse', or 'mae'")
    n_f = valid.shape[0]
    w = _weights(valid) if weighted else None
    nd = len(valid.shape)
    ax = None if axis is None else _axes(axis, nd)
    if not _on_device(valid):
        v = _host(valid)
        clim = _nanmean(v, 0)
        wh = 1. if w is None else w
        return np.array([_score_host(method, clim, v[:(n_f - f)], 0., wh, ax) for f in range(int(n_fhour))],
                        dtype=np.float64)
    from .. import ops as dops
    with device_scope(valid) as dev:
        v = _dev_operand(valid, dev)
        wt = _dev_operand(w, dev) if w is not None else None
        clim = dops.score_reduce('mean', [None, (v, tuple(int(s) for s in v.stride())), None, None], tuple(v.shape), {0},
                                 out_f32=True)
        n_lead = int(n_fhour)
        if ax is not None and 0 not in ax:
            if n_lead > 1:
                raise ValueError('the per-lead results have different shapes (the time axis is kept): cannot be stacked')
            return np.asarray(_aligned_device(method, clim.unsqueeze(0).unsqueeze(0), v.unsqueeze(0), None, wt,
                                              tuple(x + 1 for x in ax)), dtype=np.float64)
        # a = the climatology at every (lead, time); b = valid rows [0, n - f): lead stride 0
        shape = (n_lead, n_f) + _bshape(tuple(v.shape[1:]), *([tuple(wt.shape[1:]) if wt.dim() >= nd else tuple(wt.shape)]
                                                               if wt is not None else []))
        ops = [(clim, (0, 0) + _bstrides(clim, shape[2:])), (v, (0,) + _bstrides(v, shape[1:]))]
        ops.append(None)
        if wt is not None:
            ws = wt.reshape(tuple(wt.shape[1:])) if wt.dim() >= nd and wt.shape[0] == 1 else wt
            ops.append((ws, (0, 0) + _bstrides(ws, shape[2:])))
        else:
            ops.append(None)
        red = {1} | (set(range(2, len(shape))) if ax is None else set(a + 1 for a in ax if a > 0))
        out = dops.score_reduce(method, ops, shape, red, lagged=(n_f, 1))
        return np.asarray(out.cpu().numpy(), dtype=np.float64)
