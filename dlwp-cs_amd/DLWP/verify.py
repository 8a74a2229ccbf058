"""
Scoring forecasts (reference DLWP/verify.py:18-164: `forecast_error`, `persistence_error`, `climo_error`) and labelling a
cubed-sphere forecast array (behaviour of reference DLWP/verify.py:291-325, pinned by tests/golden/g11_verify.npz:
dimension names and order, coordinate values, the split of the channel axis into variable x level).

Climatologies (reference DLWP/verify.py:167-214, 426-456: `monthly_climo_error`, `daily_climatology`,
`daily_climo_time_series`): grouped means over the time axis by month or day of the year, on the device where the values lie.
`climatology_quantiles` gives grouped quantiles the same way (tercile boundaries), and `ensemble_probability`, `brier_score`,
`ranked_probability_score`, `categorical_error` and `reliability_counts` score an ensemble against them; the reference has no
counterpart of these.

The engine has no xarray: the labelled result is the `Forecast` record of DLWP.model.extensions (values, dimension names, one
coordinate array per dimension, `isel`).  `meta_ds` is anything with a `dims` mapping {name: size} and `meta_ds[name]` ->
coordinate values -- an xarray.Dataset qualifies.

The scores take the reference's arguments and give its result shapes, warnings and errors (INTEGRATION.md lists where the
engine differs: the cases the reference cannot run).  Inputs that live on a HIP device -- torch tensors, or a `Forecast` whose
values are one -- are scored by the dlwpcs_score kernel where they lie and only the score table is downloaded; numpy inputs are
scored on the host by a numpy restatement of the same formulas.  Results are float64 numpy arrays.
"""
import sys
import warnings
from collections import namedtuple

import numpy as np

from .model.extensions import Forecast

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


def _is_tensor(x):
    torch = sys.modules.get('torch')
    return torch is not None and isinstance(x, torch.Tensor)


def _raw(x):
    """the array behind a wrapped input (a Forecast / DataArray: `.values`), else x itself"""
    if isinstance(x, np.ndarray) or _is_tensor(x):
        return x
    return getattr(x, 'values', x)


def _on_device(*xs):
    return any(_is_tensor(_raw(x)) and _raw(x).is_cuda for x in xs if x is not None)


def _host(x):
    r = _raw(x)
    if hasattr(r, 'detach'):
        r = r.detach().cpu().numpy()
    return np.asarray(r)


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
            a, b = np.asarray(getattr(fc[d], 'values', fc[d])), np.asarray(getattr(vc[d], 'values', vc[d]))
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


def _axes(axis, nd):
    if axis is None:
        return None
    ax = (axis,) if isinstance(axis, (int, np.integer)) else tuple(axis)
    out = []
    for a in ax:
        a = int(a)
        if a < -nd or a >= nd:
            raise np.exceptions.AxisError(a, nd) if hasattr(np, 'exceptions') else ValueError('axis %d out of range' % a)
        out.append(a % nd)
    if len(set(out)) != len(out):
        raise ValueError('duplicate value in axis')
    return tuple(out)


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
    from . import ops as dops
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
    from . import ops as dops
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
    from . import ops as dops
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
        import torch
        dev = next(_raw(x).device for x in (forecast, valid, climatology)
                   if x is not None and isinstance(_raw(x), torch.Tensor) and _raw(x).is_cuda)
        with torch.cuda.device(dev):
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
        import torch
        dev = next(_raw(x).device for x in (forecast, valid, climatology)
                   if x is not None and isinstance(_raw(x), torch.Tensor) and _raw(x).is_cuda)
        with torch.cuda.device(dev):
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
    import torch
    dev = next(_raw(x).device for x in (a, valid) if isinstance(_raw(x), torch.Tensor) and _raw(x).is_cuda)
    with torch.cuda.device(dev):
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
    import torch
    from . import ops as dops
    dev = _raw(valid).device
    with torch.cuda.device(dev):
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


def _coord(x, name):
    c = x.coords[name]
    return np.asarray(getattr(c, 'values', c))


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
    times = _coord(ds, time_dim)
    v = _raw(ds)
    if times.shape[0] != v.shape[axis]:
        raise ValueError("the '%s' coordinate has %d entries but its axis %d" % (time_dim, times.shape[0], v.shape[axis]))
    sel = np.arange(times.shape[0]) if rows is None else np.asarray(rows, dtype=np.int64).reshape(-1)
    uniq, start, order = _csr(calendar_keys(times[sel], by))
    order = sel[order]
    if _is_tensor(v) and v.is_cuda:
        import torch
        from . import ops as dops
        with torch.cuda.device(v.device):
            src = v if v.dtype == torch.float32 else v.to(torch.float32)
            return dops.group_mean(src, start, order, row_axis=axis, out_perm=out_perm), uniq
    return _group_mean_host(_host(v), axis, start, order, out_perm), uniq


def _relabel(ds, old, new, values, coord, name):
    dims = tuple(new if d == old else d for d in ds.dims)
    coords = {}
    for d in ds.dims:
        if d == old:
            coords[new] = coord
        elif d in ds.coords:
            coords[d] = _coord(ds, d)
    out = Forecast(values, dims, coords, name=name)
    if hasattr(ds, 'lat'):
        out.lat = ds.lat
    return out


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
    return _relabel(ds, 'time', by, values, uniq, 'climatology')


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
        times = _coord(ds, 'time')
        if times.shape[0] != v.shape[axis]:
            raise ValueError("the 'time' coordinate has %d entries but its axis %d" % (times.shape[0], v.shape[axis]))
        uniq, start, order = _csr(calendar_keys(times, by))
    if _is_tensor(v) and v.is_cuda:
        import torch
        from . import ops as dops
        with torch.cuda.device(v.device):
            src = v if v.dtype == torch.float32 else v.to(torch.float32)
            values = dops.group_quantile(src, start, order, p, row_axis=axis)
    else:
        values = _group_quantile_host(_host(v), axis, start, order, p)
    out_dims, coords = ['quantile'], {'quantile': p}
    for d in dims:
        if d == 'time':
            if by is not None:
                out_dims.append(by)
                coords[by] = uniq
        else:
            out_dims.append(d)
            if d in ds.coords:
                coords[d] = _coord(ds, d)
    if by is None:
        values = values.squeeze(axis + 1)
    out = Forecast(values, tuple(out_dims), coords, name='climatology_quantiles')
    if hasattr(ds, 'lat'):
        out.lat = ds.lat
    return out


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
        if _is_tensor(t) and t.is_cuda:
            import torch
            from . import ops as dops
            with torch.cuda.device(t.device):
                src = t if t.dtype == torch.float32 else t.to(torch.float32)
                v = dops.rows_gather(src, self.rows_on(t.device), row_axis=ax).reshape(split)
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
    have = _coord(climatology, 'dayofyear').astype(np.int64)
    t = np.asarray(getattr(times, 'values', times))
    if t.dtype.kind != 'M':
        t = t.astype('datetime64[ns]')
    if f_hour is None:
        when = t
    else:
        when = t.astype('datetime64[s]')[None, :] + _lead_hours(f_hour).astype('timedelta64[s]')[:, None]
    doy = calendar_keys(when, 'dayofyear')
    rows = _sel_rows(have, doy, 'dayofyear')
    out_dims = tuple('time' if d == 'dayofyear' else d for d in dims)
    coords = {d: _coord(climatology, d) for d in dims if d != 'dayofyear' and d in climatology.coords}
    coords['time'] = t
    if f_hour is not None:
        out_dims = ('f_hour',) + out_dims
        coords['f_hour'] = np.asarray(getattr(f_hour, 'values', f_hour))
    look = ClimatologyLookup(_raw(climatology), axis, rows, out_dims, coords)
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
    times = _coord(da, time_dim)
    if climo_da is None:
        table, keys = _climatology(da, time_dim, parameter)
    else:
        want = tuple(parameter if d == time_dim else d for d in dims)
        if tuple(climo_da.dims) != want:
            raise ValueError('the climatology has dims %s, expected %s' % (tuple(climo_da.dims), want))
        table, keys = _raw(climo_da), _coord(climo_da, parameter).astype(np.int64)
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
        coords = {d: _coord(da, d) for d in dims if d in da.coords}
        coords[time_dim] = times[sel]
        return me, Forecast(anomaly, dims, coords, name='anomaly')
    return me


def _climo_error_device(method, v, table, axis, sel, rows, w, want_anomaly):
    """the score of v's rows `sel` (time axis `axis`) against the table rows `rows`, on the device: (float, anomaly or None)"""
    import torch
    from . import ops as dops
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


# --------------------------------------------------------------------------------------------------------------------- #
# Zonal spectra: scores that depend on scale
# --------------------------------------------------------------------------------------------------------------------- #
#
# RMSE and ACC reward a forecast that has smoothed its small scales away.  The zonal power spectrum shows the loss of variance
# per wavenumber, the coherence how much of the verification's phase the forecast still holds at each scale.  For a row
# x[0..L-1] along longitude:  X_k = sum_j x_j exp(-2 pi i jk / L),  P_k = c_k |X_k|^2 / L^2 with c_k = 1 for k = 0 and for
# k = L/2 when L is even, else 2 -- so that sum_k P_k = mean_j x_j^2.  Rows are averaged with weights; a row counts only when all
# of its values are finite (in both arrays of a pair).  numpy inputs are transformed on the host (np.fft.rfft in float64),
# device tensors by dlwpcs_zonal_spectrum; neither path falls back to the other.

CrossSpectrum = namedtuple('CrossSpectrum', ['power_f', 'power_v', 'co', 'quad'])


def _lon_axis(x, lon_axis):
    """the longitude axis: the dim named 'lon' of a labelled input, else `lon_axis`"""
    nd = len(x.shape)
    if hasattr(x, 'dims') and 'lon' in tuple(x.dims):
        return tuple(x.dims).index('lon')
    a = int(lon_axis)
    if a < -nd or a >= nd:
        raise ValueError('lon_axis %d out of range of %d axes' % (a, nd))
    return a % nd


def _spectrum_axes(x, axis, lon):
    """the averaged axes of x: all but longitude for None; ints, or dim names of a labelled input"""
    nd = len(x.shape)
    if axis is None:
        return tuple(i for i in range(nd) if i != lon)
    ax = (axis,) if isinstance(axis, (int, np.integer, str)) else tuple(axis)
    ax = tuple(tuple(x.dims).index(a) if isinstance(a, str) else a for a in ax)
    ax = _axes(ax, nd)
    if lon in ax:
        raise ValueError('the longitude axis is transformed, it cannot be averaged over')
    return ax


def _row_weights(x, lon, weighted, weights):
    """float64 weights that broadcast against the leading shape (x's shape without longitude), or None"""
    lead = tuple(int(e) for i, e in enumerate(x.shape) if i != lon)
    w = None
    if weighted:
        full = np.asarray(_weights(x), dtype=np.float64)
        shape = tuple(int(e) for e in x.shape)
        full = full.reshape((1,) * (len(shape) - full.ndim) + full.shape) if full.ndim <= len(shape) else full
        if full.ndim != len(shape) or full.shape[lon] != 1 or any(e not in (1, s) for e, s in zip(full.shape, shape)):
            raise ValueError('the latitude weights %s must broadcast against %s and be constant along longitude'
                             % (full.shape, shape))
        w = np.squeeze(full, axis=lon)
    if weights is not None:
        ex = np.asarray(_host(weights), dtype=np.float64)
        np.broadcast_shapes(ex.shape, lead)                   # raises where they do not fit
        if ex.ndim > len(lead):
            raise ValueError('weights %s have more axes than the leading shape %s' % (ex.shape, lead))
        w = ex if w is None else w * ex
    if w is not None and not np.all(np.isfinite(w)):
        raise ValueError('the weights must be finite')
    return w


def _spectrum_host(f, v, lon, ax, w, n_wave, remove_mean):
    """numpy twin of dlwpcs_zonal_spectrum: (quantities (nq, kept..., K) float64, skipped rows (kept...) int32)"""
    arrs = [np.moveaxis(np.asarray(x, dtype=np.float64), lon, -1) for x in ((f,) if v is None else (f, v))]
    L = arrs[0].shape[-1]
    K = L // 2 + 1 if n_wave is None else int(n_wave)
    lead = arrs[0].shape[:-1]
    red = tuple(a if a < lon else a - 1 for a in ax)
    counted = np.ones(lead, dtype=bool)
    for x in arrs:
        counted &= np.isfinite(x).all(axis=-1)
    ck = np.full(K, 2.0)
    ck[0] = 1.0
    if L % 2 == 0 and K == L // 2 + 1:
        ck[-1] = 1.0
    spec, means = [], []
    for x in arrs:
        x = np.where(counted[..., None], x, 0.0)
        m = x.mean(axis=-1)
        means.append(m)
        spec.append(np.fft.rfft(x - m[..., None] if remove_mean else x, axis=-1)[..., :K])
    F, V = spec[0], spec[-1]
    q = [ck * (F.real ** 2 + F.imag ** 2) / L ** 2]
    if v is not None:
        cross = F * np.conj(V)
        q += [ck * (V.real ** 2 + V.imag ** 2) / L ** 2, ck * cross.real / L ** 2, ck * cross.imag / L ** 2]
    if remove_mean:
        q[0][..., 0] = means[0] ** 2
        if v is not None:
            q[1][..., 0], q[2][..., 0], q[3][..., 0] = means[1] ** 2, means[0] * means[1], 0.0
    wf = np.broadcast_to(1.0 if w is None else w, lead) * counted
    sw = wf.sum(axis=red) if red else wf.copy()
    with np.errstate(invalid='ignore', divide='ignore'):
        out = np.stack([np.where(sw[..., None] == 0, np.nan, (x * wf[..., None]).sum(axis=red) / sw[..., None]) for x in q])
    skipped = (~counted).sum(axis=red) if red else (~counted).astype(np.int64)
    return out, np.asarray(skipped, dtype=np.int32)


def _spectrum_device(f, v, lon, ax, w, n_wave, remove_mean):
    import torch
    from . import ops as dops
    dev = next(_raw(x).device for x in (f, v) if x is not None and _is_tensor(_raw(x)) and _raw(x).is_cuda)
    with torch.cuda.device(dev):
        ft = _dev_operand(f, dev)
        vt = _dev_operand(v, dev) if v is not None else None
        wt = _dev_operand(w, dev) if w is not None else None
        out, cnt = dops.zonal_spectrum(ft, vt, lon_axis=lon, reduced=ax, weights=wt, n_wave=n_wave, remove_mean=remove_mean,
                                       counts=True)
        out = out.cpu().numpy().astype(np.float64)
        return (out[None] if v is None else out), cnt.cpu().numpy()


def _spectrum(f, v, lon_axis, axis, weighted, weights, n_wave, remove_mean):
    """(quantities (nq, kept..., K) float64, skipped, kept dim names or None, lon axis)"""
    if v is not None:
        if len(v.shape) == len(f.shape) - 1:
            raise NotImplementedError('the lagged form against a continuous verification series (valid[f + t]) is not served: '
                                      'aligned arrays of one shape are')
        _check_labels(f, v)
        if tuple(f.shape) != tuple(v.shape):
            raise ValueError('forecast %s and verification %s must have one shape' % (tuple(f.shape), tuple(v.shape)))
    if len(f.shape) < 1:
        raise ValueError('the input needs a longitude axis')
    lon = _lon_axis(f, lon_axis)
    L = int(f.shape[lon])
    if L < 2:
        raise ValueError('%d longitudes (at least 2)' % L)
    if n_wave is not None and not 1 <= int(n_wave) <= L // 2 + 1:
        raise ValueError('n_wave = %s outside 1 .. L // 2 + 1 = %d' % (n_wave, L // 2 + 1))
    ax = _spectrum_axes(f, axis, lon)
    w = _row_weights(f if v is None else v, lon, weighted, weights)
    if _on_device(f, v):
        out, skipped = _spectrum_device(f, v, lon, ax, w, n_wave, remove_mean)
    else:
        out, skipped = _spectrum_host(_host(f), None if v is None else _host(v), lon, ax, w, n_wave, remove_mean)
    dims = None
    if hasattr(f, 'dims'):
        dims = tuple(d for i, d in enumerate(f.dims) if i != lon and i not in ax)
    return out, skipped, dims, f


def _label(values, dims, src, name):
    """a Forecast over the kept dims of `src` plus 'wavenumber' when the input was labelled, else the array"""
    if dims is None:
        return values
    coords = {d: np.asarray(getattr(src.coords[d], 'values', src.coords[d])) for d in dims if d in getattr(src, 'coords', {})}
    coords['wavenumber'] = np.arange(values.shape[-1])
    return Forecast(values, dims + ('wavenumber',), coords, name=name)


def zonal_spectrum(x, lon_axis=-1, axis=None, weighted=False, weights=None, n_wave=None, remove_mean=False, return_count=False):
    """
    One-sided zonal power spectrum P_k = c_k |X_k|^2 / L^2 of `x` along longitude, averaged over `axis`.

    :param x: ndarray, device tensor or labelled array (its dim 'lon' is the longitude axis)
    :param lon_axis: the longitude axis of an unlabelled input
    :param axis: int, dim name, tuple or None: the axes averaged over besides longitude, which is transformed (None: all)
    :param weighted: weight the rows by cos(latitude) read from `x.lat`
    :param weights: row weights that broadcast against the leading axes (x's shape without longitude); a latitude band is a
        weight of zeros and ones, times cos(latitude) where wanted.  Multiplies the cos(latitude) weights of `weighted`.
    :param n_wave: return the first n_wave wavenumbers only (1 .. L // 2 + 1)
    :param remove_mean: subtract each row's zonal mean before the transform and report P_0 as that mean squared: the same
        numbers, but the rounding error of the other wavenumbers no longer scales with the offset squared (280 K temperatures)
    :param return_count: also return the number of rows per result that did not count (rows holding a NaN or an infinity)
    :return: float64 array (kept axes..., wavenumber), labelled like the input; NaN where no row counts or the weights sum to 0
    """
    out, skipped, dims, src = _spectrum(x, None, lon_axis, axis, weighted, weights, n_wave, remove_mean)
    res = _label(out[0], dims, src, 'zonal_spectrum')
    return (res, skipped) if return_count else res


def zonal_cross_spectrum(forecast, valid, lon_axis=-1, axis=None, weighted=False, weights=None, n_wave=None, remove_mean=False,
                         return_count=False):
    """
    Zonal power spectra of a forecast and its verification (aligned arrays of one shape) and their cross-spectrum, averaged
    over `axis`: CrossSpectrum(power_f, power_v, co, quad) with co + i quad = c_k F_k conj(V_k) / L^2.  A row counts only when
    it is finite in both arrays.  Arguments as for `zonal_spectrum`; a continuous verification series (one axis fewer) raises
    NotImplementedError.
    """
    out, skipped, dims, src = _spectrum(forecast, valid, lon_axis, axis, weighted, weights, n_wave, remove_mean)
    res = CrossSpectrum(*[_label(out[i], dims, src, n) for i, n in enumerate(CrossSpectrum._fields)])
    return (res, skipped) if return_count else res


def zonal_coherence(forecast, valid, lon_axis=-1, axis=None, weighted=False, weights=None, n_wave=None, remove_mean=False,
                    return_count=False):
    """
    Squared coherence (co^2 + quad^2) / (power_f power_v) per wavenumber, formed from the AVERAGED spectra of
    `zonal_cross_spectrum` (per row it would be identically 1): 1 where the forecast holds the verification's phase over the
    averaged rows, near 1 / rows where the two are unrelated.  NaN where either power is 0.  Arguments as for `zonal_spectrum`.
    """
    out, skipped, dims, src = _spectrum(forecast, valid, lon_axis, axis, weighted, weights, n_wave, remove_mean)
    with np.errstate(invalid='ignore', divide='ignore'):
        coh = (out[2] ** 2 + out[3] ** 2) / (out[0] * out[1])
    res = _label(coh, dims, src, 'zonal_coherence')
    return (res, skipped) if return_count else res


# --------------------------------------------------------------------------------------------------------------------- #
# Spherical-harmonic spectra: power per total wavenumber
# --------------------------------------------------------------------------------------------------------------------- #
#
# The zonal spectrum treats a row at 80 N like a row at the equator and names no scale in kilometres.  The spherical-harmonic
# spectrum S_n = sum_{m<=n} c_m |a_n^m|^2 (DLWP/remap/spharm.py states the definitions) is the power per total wavenumber n that
# the literature reports: sum_n S_n is the area-weighted mean square of a band-limited field, S_0 its squared global mean, and
# degree n is a wavelength of 40 000 km / n.  The latitudes must be Gaussian, equally spaced with both poles, or equally spaced
# cell centres; the area weighting is inside the transform.  numpy inputs are transformed on the host (np.fft.rfft and the float64
# Legendre table), device tensors by dlwpcs_sht_spectrum; neither path falls back to the other.

SphericalCrossSpectrum = namedtuple('SphericalCrossSpectrum', ['power_f', 'power_v', 'co'])
_transforms = {}


def _spherical_transform(lat, n_lon, truncation):
    from .remap.spharm import SphericalTransform
    lat = np.asarray(_host(lat), dtype=np.float64).reshape(-1)
    key = (lat.tobytes(), int(n_lon), None if truncation is None else int(truncation))
    hit = _transforms.get(key)
    if hit is None:
        hit = _transforms[key] = SphericalTransform(lat, n_lon, truncation)
    return hit


def _grid_axis(x, name, given):
    nd = len(x.shape)
    if hasattr(x, 'dims') and name in tuple(x.dims):
        return tuple(x.dims).index(name)
    a = int(given)
    if a < -nd or a >= nd:
        raise ValueError('%s_axis %d out of range of %d axes' % (name, a, nd))
    return a % nd


def _sht_host(f, v, la, lo, ax, tr):
    """numpy twin of ops.spherical_spectrum: (quantities (nq, kept..., T + 1) float64, skipped fields (kept...) int32)"""
    arrs = [np.moveaxis(np.asarray(x, dtype=np.float64), (la, lo), (-2, -1)) for x in ((f,) if v is None else (f, v))]
    lead_axes = [i for i in range(arrs[0].ndim) if i not in (la, lo)]
    red = tuple(lead_axes.index(a) for a in ax)
    counted = np.ones(arrs[0].shape[:-2], dtype=bool)
    for x in arrs:
        counted &= np.isfinite(x).all(axis=(-2, -1))
    arrs = [np.where(counted[..., None, None], x, 0.0) for x in arrs]
    q = tr.power(arrs[0], None if v is None else arrs[1])
    n = counted.sum(axis=red) if red else counted.astype(np.int64)
    with np.errstate(invalid='ignore', divide='ignore'):
        total = (q * counted[..., None]).sum(axis=tuple(r + 1 for r in red)) if red else q * counted[..., None]
        out = np.where(n[..., None] == 0, np.nan, total / np.maximum(n, 1)[..., None])
    skipped = (~counted).sum(axis=red) if red else (~counted).astype(np.int64)
    return out, np.asarray(skipped, dtype=np.int32)


def _sht_grid(f, lat, lat_axis, lon_axis, truncation):
    """(latitude axis, longitude axis, SphericalTransform) of the input f"""
    if len(f.shape) < 2:
        raise ValueError('the input needs a latitude and a longitude axis')
    la, lo = _grid_axis(f, 'lat', lat_axis), _grid_axis(f, 'lon', lon_axis)
    if la == lo:
        raise ValueError('the latitude and the longitude axis must differ')
    if lat is None:
        coords = getattr(f, 'coords', {})
        lat = coords['lat'] if 'lat' in coords else getattr(f, 'lat', None)
        if lat is None:
            raise ValueError("the latitudes are needed: pass lat=, or a labelled input with a 'lat' coordinate")
    lat = np.asarray(_host(lat), dtype=np.float64).reshape(-1)
    if lat.size != int(f.shape[la]):
        raise ValueError('%d latitudes for a latitude axis of %d' % (lat.size, int(f.shape[la])))
    return la, lo, _spherical_transform(lat, int(f.shape[lo]), truncation)


def _sht(f, v, lat, lat_axis, lon_axis, axis, truncation):
    """(quantities (nq, kept..., T + 1) float64, skipped, kept dim names or None)"""
    if v is not None:
        if len(v.shape) == len(f.shape) - 1:
            raise NotImplementedError('the lagged form against a continuous verification series (valid[f + t]) is not served: '
                                      'aligned arrays of one shape are')
        _check_labels(f, v)
        if tuple(f.shape) != tuple(v.shape):
            raise ValueError('forecast %s and verification %s must have one shape' % (tuple(f.shape), tuple(v.shape)))
    la, lo, tr = _sht_grid(f, lat, lat_axis, lon_axis, truncation)
    nd = len(f.shape)
    if axis is None:
        ax = tuple(i for i in range(nd) if i not in (la, lo))
    else:
        ax = (axis,) if isinstance(axis, (int, np.integer, str)) else tuple(axis)
        ax = _axes(tuple(tuple(f.dims).index(a) if isinstance(a, str) else a for a in ax), nd)
        if la in ax or lo in ax:
            raise ValueError('the latitude and longitude axes are transformed, they cannot be averaged over')
    if _on_device(f, v):
        import torch
        from . import ops as dops
        dev = next(_raw(x).device for x in (f, v) if x is not None and _is_tensor(_raw(x)) and _raw(x).is_cuda)
        with torch.cuda.device(dev):
            ft = _dev_operand(f, dev)
            vt = _dev_operand(v, dev) if v is not None else None
            out, cnt = dops.spherical_spectrum(ft, vt, transform=tr, lat_axis=la, lon_axis=lo, reduced=ax, counts=True)
            out = out.cpu().numpy().astype(np.float64)
            out, skipped = (out[None] if v is None else out), cnt.cpu().numpy()
    else:
        out, skipped = _sht_host(_host(f), None if v is None else _host(v), la, lo, ax, tr)
    dims = tuple(d for i, d in enumerate(f.dims) if i not in (la, lo) and i not in ax) if hasattr(f, 'dims') else None
    return out, skipped, dims


def _label_degree(values, dims, src, name):
    """a Forecast over the kept dims of `src` plus 'degree' when the input was labelled, else the array"""
    if dims is None:
        return values
    coords = {d: np.asarray(getattr(src.coords[d], 'values', src.coords[d])) for d in dims if d in getattr(src, 'coords', {})}
    coords['degree'] = np.arange(values.shape[-1])
    return Forecast(values, dims + ('degree',), coords, name=name)


def spherical_spectrum(x, lat=None, lat_axis=-2, lon_axis=-1, axis=None, truncation=None, return_count=False):
    """
    Spherical-harmonic power spectrum S_n = sum_{m<=n} c_m |a_n^m|^2 of `x`, n = 0 .. truncation, averaged over `axis`.

    There is no `weighted=` argument: the area weighting is inside the transform (the quadrature weights of the latitudes).

    :param x: ndarray, device tensor or labelled array (its dims 'lat' and 'lon' are the grid axes, its coordinate 'lat' the
        latitudes)
    :param lat: the latitudes in degrees, either direction: Gaussian, equally spaced with both poles (181 latitudes), or equally
        spaced cell centres; any other vector is refused.  Needed for unlabelled inputs.
    :param lat_axis, lon_axis: the grid axes of an unlabelled input
    :param axis: int, dim name, tuple or None: the axes averaged over (None: all but the grid axes).  A field counts only when
        all of its values are finite.
    :param truncation: the largest degree; None: the largest the grid allows -- nlat - 1 for Gaussian latitudes,
        (nlat - 1) // 2 for the equally spaced ones, and (n_lon - 1) // 2.  A larger one is a ValueError.
    :param return_count: also return the number of fields per result that did not count
    :return: float64 array (kept axes..., degree), labelled like the input; NaN where no field counts
    """
    out, skipped, dims = _sht(x, None, lat, lat_axis, lon_axis, axis, truncation)
    res = _label_degree(out[0], dims, x, 'spherical_spectrum')
    return (res, skipped) if return_count else res


def spherical_cross_spectrum(forecast, valid, lat=None, lat_axis=-2, lon_axis=-1, axis=None, truncation=None, return_count=False):
    """
    Spherical-harmonic spectra of a forecast and its verification (aligned arrays of one shape) and their co-spectrum, averaged
    over `axis`: SphericalCrossSpectrum(power_f, power_v, co) with co_n = sum_m c_m Re(a_n^m(f) conj a_n^m(v)).  The imaginary
    part is not invariant under rotations and is not returned.  A field counts only when it is finite in both arrays.  Arguments as
    for `spherical_spectrum`; a continuous verification series (one axis fewer) raises NotImplementedError.
    """
    out, skipped, dims = _sht(forecast, valid, lat, lat_axis, lon_axis, axis, truncation)
    res = SphericalCrossSpectrum(*[_label_degree(out[i], dims, forecast, n) for i, n in enumerate(SphericalCrossSpectrum._fields)])
    return (res, skipped) if return_count else res


def spherical_correlation(forecast, valid, lat=None, lat_axis=-2, lon_axis=-1, axis=None, truncation=None, return_count=False):
    """
    Correlation per degree co / sqrt(power_f power_v), formed from the AVERAGED quantities of `spherical_cross_spectrum`: the
    anomaly correlation of the two fields restricted to total wavenumber n.  NaN where either power is 0.  Arguments as for
    `spherical_spectrum`.
    """
    out, skipped, dims = _sht(forecast, valid, lat, lat_axis, lon_axis, axis, truncation)
    with np.errstate(invalid='ignore', divide='ignore'):
        cor = out[2] / np.sqrt(out[0] * out[1])
    res = _label_degree(cor, dims, forecast, 'spherical_correlation')
    return (res, skipped) if return_count else res


# --------------------------------------------------------------------------------------------------------------------- #
# Spherical-harmonic analysis, synthesis and filtering
# --------------------------------------------------------------------------------------------------------------------- #
#
# The coefficients themselves, the inverse transform, and the chain analysis -> factor per degree -> synthesis: truncation to a
# coarser resolution (scale-separated verification: forecast_error(spherical_filter(f, cutoff=21), spherical_filter(v, cutoff=21))),
# the Laplacian and its inverse (height <-> vorticity), smoothing before a remap.  numpy inputs run on the host in float64 and
# return numpy; device tensors run through dlwpcs_sht_analysis / dlwpcs_sht_synthesis and return device tensors (float32 /
# complex64); neither path falls back to the other.  A field that holds a NaN or an infinity has NaN coefficients and comes back
# as a field of NaN.

_responses = {}             # (response bytes, device) -> float32 device vector


def _device_of(x):
    return _raw(x).device


def _response_on(response, dev):
    """the float32 device copy of a host response, uploaded once per device (so that a later call can be captured)"""
    import torch
    if response is None or _is_tensor(response):
        return response
    r32 = np.ascontiguousarray(np.asarray(response, dtype=np.float64).reshape(-1).astype(np.float32))
    key = (r32.tobytes(), str(dev))
    hit = _responses.get(key)
    if hit is None:
        if torch.cuda.is_current_stream_capturing():
            from . import _native as nat
            raise nat.NativeError('spherical_filter: first use of this response inside a graph capture (run it once eagerly first)')
        hit = _responses[key] = torch.from_numpy(r32).to(dev)
    return hit


def _coef_dims(x, la, lo):
    return tuple(d for i, d in enumerate(x.dims) if i not in (la, lo)) if hasattr(x, 'dims') else None


def _sht_label(values, dims, src, name):
    """a Forecast over `dims` with the coordinates `src` has for them when the input was labelled, else the array"""
    if dims is None:
        return values
    coords = {d: np.asarray(getattr(src.coords[d], 'values', src.coords[d])) for d in dims if d in getattr(src, 'coords', {})}
    return Forecast(values, dims, coords, name=name)


def _analysis_host(x, la, lo, tr):
    """(complex128 coefficients (lead..., rows), int32 flags (lead...)) of the host array x"""
    arr = np.moveaxis(np.asarray(x, dtype=np.float64), (la, lo), (-2, -1))
    counted = np.isfinite(arr).all(axis=(-2, -1))
    coef = tr.coefficients(np.where(counted[..., None, None], arr, 0.0))
    coef[~counted] = complex(np.nan, np.nan)
    return coef, (~counted).astype(np.int32)


def spherical_analysis(x, lat=None, lat_axis=-2, lon_axis=-1, truncation=None, return_count=False):
    """
    The spherical-harmonic coefficients a_n^m of `x`, 0 <= m <= n <= truncation (DLWP/remap/spharm.py states the definitions).

    :param x: ndarray, device tensor or labelled array; grid axes, `lat` and `truncation` as for `spherical_spectrum`
    :param return_count: also return an int32 array (leading axes...) that holds 1 for a field with a NaN or an infinity
    :return: complex array (leading axes..., (T + 1)(T + 2) / 2) in the order of spharm.packed_row(m, n, T): complex128 numpy for
        host inputs, a complex64 device tensor for device inputs; a labelled input gives a Forecast whose last dim is
        'coefficient'.  A field that holds a NaN or an infinity has NaN coefficients.
    """
    la, lo, tr = _sht_grid(x, lat, lat_axis, lon_axis, truncation)
    if _on_device(x):
        import torch
        from . import ops as dops
        dev = _device_of(x)
        with torch.cuda.device(dev):
            coef, flags = dops.spherical_analysis(_dev_operand(x, dev), tr, lat_axis=la, lon_axis=lo, counts=True)
    else:
        coef, flags = _analysis_host(_host(x), la, lo, tr)
    dims = _coef_dims(x, la, lo)
    res = _sht_label(coef, None if dims is None else dims + ('coefficient',), x, 'spherical_analysis')
    return (res, flags) if return_count else res


def _truncation_of_rows(rows):
    T = int(round((np.sqrt(8.0 * rows + 1.0) - 3.0) / 2.0))
    if T < 0 or (T + 1) * (T + 2) // 2 != rows:
        raise ValueError('%d coefficients per field are not (T + 1)(T + 2) / 2 for any truncation T' % rows)
    return T


def spherical_synthesis(coef, lat, n_lon, response=None):
    """
    The fields x[i, j] = sum_m c_m Re(e^{i m lon_j} sum_n r_n a_n^m Pbar_n^m(mu_i)) of the coefficients `coef`
    (leading axes..., (T + 1)(T + 2) / 2), as `spherical_analysis` returns them, on the latitudes `lat` (degrees) and n_lon longitudes.

    :param coef: complex ndarray, complex64 device tensor or labelled array (its last dim holds the coefficients)
    :param response: T + 1 real factors per degree (None: ones); see spharm.truncation_response, spharm.laplacian_response
    :return: (leading axes..., nlat, n_lon): float64 numpy for host inputs, a float32 device tensor for device inputs; a labelled
        input gives a Forecast with the dims 'lat' and 'lon' in place of the coefficient dim
    """
    if len(coef.shape) < 1:
        raise ValueError('the coefficients need an axis')
    T = _truncation_of_rows(int(coef.shape[-1]))
    tr = _spherical_transform(lat, n_lon, T)
    if response is not None and not _is_tensor(response) and np.asarray(response).size != T + 1:
        raise ValueError('a response of %d factors, truncation %d needs %d' % (np.asarray(response).size, T, T + 1))
    if _on_device(coef):
        import torch
        from . import ops as dops
        dev = _device_of(coef)
        with torch.cuda.device(dev):
            c = _raw(coef)
            out = dops.spherical_synthesis(c if c.dtype == torch.complex64 else c.to(torch.complex64), tr, _response_on(response, dev))
    else:
        out = tr.synthesis(_host(coef), None if response is None else _host(response))
    if not hasattr(coef, 'dims'):
        return out
    dims = tuple(coef.dims)[:-1] + ('lat', 'lon')
    coords = {d: np.asarray(getattr(coef.coords[d], 'values', coef.coords[d])) for d in dims if d in getattr(coef, 'coords', {})}
    coords['lat'] = tr.lat.copy()
    coords['lon'] = np.arange(tr.n_lon) * 360.0 / tr.n_lon
    return Forecast(out, dims, coords, name='spherical_synthesis')


def _filter(x, lat, lat_axis, lon_axis, truncation, response, name):
    """analysis, `response` (a function of the transform's truncation, or None) and synthesis back into x's shape and axis order"""
    la, lo, tr = _sht_grid(x, lat, lat_axis, lon_axis, truncation)
    T = tr.truncation
    r = response(T) if callable(response) else response
    if r is not None and not _is_tensor(r) and np.asarray(r).size != T + 1:
        raise ValueError('a response of %d factors, truncation %d needs %d' % (np.asarray(r).size, T, T + 1))
    nd = len(x.shape)
    lead_axes = [i for i in range(nd) if i not in (la, lo)]
    if _on_device(x):
        import torch
        from . import ops as dops
        dev = _device_of(x)
        with torch.cuda.device(dev):
            xt = _dev_operand(x, dev)
            coef = dops.spherical_analysis(xt, tr, lat_axis=la, lon_axis=lo)
            # the result has x's shape and axis order, and longitude at unit stride whatever x's own layout
            order = [i for i in range(nd) if i != lo] + [lo]
            buf = torch.empty([int(xt.shape[i]) for i in order], dtype=torch.float32, device=dev)
            out = buf.permute([order.index(i) for i in range(nd)])
            dops.spherical_synthesis(coef, tr, _response_on(r, dev), out=out.permute(lead_axes + [la, lo]))
    else:
        coef, _ = _analysis_host(_host(x), la, lo, tr)
        out = np.moveaxis(tr.synthesis(coef, None if r is None else _host(r)), (-2, -1), (la, lo))
    return _sht_label(out, tuple(x.dims) if hasattr(x, 'dims') else None, x, name)


def spherical_filter(x, lat=None, lat_axis=-2, lon_axis=-1, truncation=None, cutoff=None, response=None):
    """
    `x` with every spherical-harmonic degree n multiplied by a real factor: analysis up to `truncation`, the factor, synthesis.

    :param x: ndarray, device tensor or labelled array; grid axes, `lat` and `truncation` as for `spherical_spectrum`
    :param cutoff: keep the degrees n <= cutoff and drop the others (the field truncated to T`cutoff`)
    :param response: truncation + 1 real factors per degree (host array, or a float32 device vector for device inputs);
        `cutoff` and `response` are mutually exclusive, neither: the field band-limited to `truncation`
    :return: the filtered field with the shape, axis order and labels of `x`: float64 numpy for host inputs, a float32 device tensor
        for device inputs (four launches; after one eager call the call can be captured in a graph)
    """
    if cutoff is not None and response is not None:
        raise ValueError('cutoff and response are mutually exclusive')
    if cutoff is not None:
        from .remap.spharm import truncation_response
        cut = int(cutoff)
        if cut < 0:
            raise ValueError('cutoff %d is negative' % cut)
        response = lambda T: truncation_response(T, cut)        # noqa: E731
    return _filter(x, lat, lat_axis, lon_axis, truncation, response, 'spherical_filter')


def spherical_laplacian(x, lat=None, lat_axis=-2, lon_axis=-1, truncation=None, radius=6371200., inverse=False):
    """
    The Laplacian of `x` on a sphere of `radius` metres, degree n multiplied by -n (n + 1) / radius^2 (height -> vorticity up to
    g / f); inverse=True: the inverse Laplacian, degree n >= 1 divided by that factor and the mean set to 0.  Arguments and
    result as for `spherical_filter`.
    """
    from .remap.spharm import laplacian_response
    return _filter(x, lat, lat_axis, lon_axis, truncation, lambda T: laplacian_response(T, radius, inverse), 'spherical_laplacian')


# --------------------------------------------------------------------------------------------------------------------- #
# Vector spherical harmonics: winds, vorticity and divergence, gradients
# --------------------------------------------------------------------------------------------------------------------- #
#
# Winds from vorticity and divergence, vorticity and divergence from winds, and the gradient of a scalar, on a sphere of `radius`
# metres (DLWP/remap/spharm.py states the definitions).  numpy inputs run on the host in float64, device tensors through
# dlwpcs_sht_vector_synthesis / dlwpcs_sht_vector_analysis (float32 / complex64, device tensors come back); neither path falls
# back to the other.

def _uv_response(T, radius, dev=None):
    from .remap.spharm import uv_response
    r = uv_response(T, radius)
    return r if dev is None else _response_on(r, dev)


def _grid_forecast(values, src, tr, name):
    """a Forecast of grid fields over the dims of the coefficients `src` with 'lat' and 'lon' in place of the coefficient dim"""
    dims = tuple(src.dims)[:-1] + ('lat', 'lon')
    coords = {d: np.asarray(getattr(src.coords[d], 'values', src.coords[d])) for d in dims if d in getattr(src, 'coords', {})}
    coords['lat'] = tr.lat.copy()
    coords['lon'] = np.arange(tr.n_lon) * 360.0 / tr.n_lon
    return Forecast(values, dims, coords, name=name)


def spherical_uv(vrt, div, lat, n_lon, radius=6371200.):
    """
    The wind (u, v) whose vorticity and divergence have the coefficients `vrt` and `div` (leading axes..., (T + 1)(T + 2) / 2), as
    `spherical_vrtdiv` returns them, on the latitudes `lat` (degrees) and n_lon longitudes: psi = lap^-1 vrt, chi = lap^-1 div,
    u = -dpsi/dphi / radius + dchi/dlambda / (radius cos), v = dpsi/dlambda / (radius cos) + dchi/dphi / radius.

    :param vrt, div: complex ndarrays, complex64 device tensors or labelled arrays of one shape; either may be None (taken as zero)
    :return: (u, v), each (leading axes..., nlat, n_lon): float64 numpy for host inputs, float32 device tensors for device inputs,
        Forecasts with the dims 'lat' and 'lon' in place of the coefficient dim for labelled inputs
    """
    if vrt is None and div is None:
        raise ValueError('spherical_uv: vorticity and divergence are both absent')
    first = vrt if vrt is not None else div
    if vrt is not None and div is not None and tuple(vrt.shape) != tuple(div.shape):
        raise ValueError('spherical_uv: vorticity %s and divergence %s must have one shape' % (tuple(vrt.shape), tuple(div.shape)))
    if len(first.shape) < 1:
        raise ValueError('the coefficients need an axis')
    T = _truncation_of_rows(int(first.shape[-1]))
    tr = _spherical_transform(lat, n_lon, T)
    if _on_device(*[c for c in (vrt, div) if c is not None]):
        import torch
        from . import ops as dops
        dev = _device_of(first)
        with torch.cuda.device(dev):
            cs = [None if c is None else (_raw(c) if _raw(c).dtype == torch.complex64 else _raw(c).to(torch.complex64)) for c in (vrt, div)]
            r = _uv_response(T, radius, dev)
            u, v = dops.spherical_vector_synthesis(cs[0], cs[1], tr, r, r)
    else:
        u, v = tr.uv_from_vrtdiv(None if vrt is None else _host(vrt), None if div is None else _host(div), radius)
    if not hasattr(first, 'dims'):
        return u, v
    return _grid_forecast(u, first, tr, 'u'), _grid_forecast(v, first, tr, 'v')


def spherical_vrtdiv(u, v, lat=None, lat_axis=-2, lon_axis=-1, truncation=None, radius=6371200.):
    """
    The coefficients (vrt, div) of the vorticity and the divergence of the wind (u, v) on a sphere of `radius` metres.

    :param u, v: ndarrays, device tensors or labelled arrays of one shape; grid axes, `lat` and `truncation` as for
        `spherical_spectrum`
    :return: (vrt, div), complex (leading axes..., (T + 1)(T + 2) / 2) as `spherical_analysis` returns coefficients.  A field with
        a NaN or an infinity in u or in v has NaN coefficients in both.
    """
    _check_labels(u, v)
    if tuple(u.shape) != tuple(v.shape):
        raise ValueError('spherical_vrtdiv: u %s and v %s must have one shape' % (tuple(u.shape), tuple(v.shape)))
    la, lo, tr = _sht_grid(u, lat, lat_axis, lon_axis, truncation)
    if _on_device(u, v):
        import torch
        from . import ops as dops
        dev = next(_raw(x).device for x in (u, v) if _is_tensor(_raw(x)) and _raw(x).is_cuda)
        with torch.cuda.device(dev):
            r = _response_on(np.full(tr.truncation + 1, 1.0 / float(radius)), dev)
            vrt, div = dops.spherical_vector_analysis(_dev_operand(u, dev), _dev_operand(v, dev), tr, r, lat_axis=la, lon_axis=lo)
    else:
        arrs = [np.moveaxis(np.asarray(_host(x), dtype=np.float64), (la, lo), (-2, -1)) for x in (u, v)]
        counted = np.isfinite(arrs[0]).all(axis=(-2, -1)) & np.isfinite(arrs[1]).all(axis=(-2, -1))
        arrs = [np.where(counted[..., None, None], x, 0.0) for x in arrs]
        vrt, div = tr.vrtdiv_from_uv(arrs[0], arrs[1], radius)
        vrt[~counted] = complex(np.nan, np.nan)
        div[~counted] = complex(np.nan, np.nan)
    dims = _coef_dims(u, la, lo)
    dims = None if dims is None else dims + ('coefficient',)
    return _sht_label(vrt, dims, u, 'vorticity'), _sht_label(div, dims, u, 'divergence')


def spherical_gradient(x, lat=None, lat_axis=-2, lon_axis=-1, truncation=None, radius=6371200.):
    """
    The gradient (dx/dlambda / (radius cos(phi)), dx/dphi / radius) of the scalar `x` on a sphere of `radius` metres: analysis up
    to `truncation`, then the vector synthesis of the potential chi = x.  Arguments as for `spherical_filter`; the two results
    have the shape, axis order and labels of `x`.
    """
    la, lo, tr = _sht_grid(x, lat, lat_axis, lon_axis, truncation)
    T = tr.truncation
    nd = len(x.shape)
    lead_axes = [i for i in range(nd) if i not in (la, lo)]
    if _on_device(x):
        import torch
        from . import ops as dops
        dev = _device_of(x)
        with torch.cuda.device(dev):
            xt = _dev_operand(x, dev)
            coef = dops.spherical_analysis(xt, tr, lat_axis=la, lon_axis=lo)
            order = [i for i in range(nd) if i != lo] + [lo]
            outs = []
            for _ in range(2):
                buf = torch.empty([int(xt.shape[i]) for i in order], dtype=torch.float32, device=dev)
                outs.append(buf.permute([order.index(i) for i in range(nd)]))
            r = _response_on(np.full(T + 1, 1.0 / float(radius)), dev)
            dops.spherical_vector_synthesis(None, coef, tr, None, r, out_u=outs[0].permute(lead_axes + [la, lo]),
                                            out_v=outs[1].permute(lead_axes + [la, lo]))
    else:
        coef, _ = _analysis_host(_host(x), la, lo, tr)
        outs = [np.moveaxis(g, (-2, -1), (la, lo)) for g in tr.gradient(coef, radius)]
    dims = tuple(x.dims) if hasattr(x, 'dims') else None
    return _sht_label(outs[0], dims, x, 'gradient_lon'), _sht_label(outs[1], dims, x, 'gradient_lat')


# --------------------------------------------------------------------------------------------------------------------- #
# Ensembles: probabilistic scores over a member axis
# --------------------------------------------------------------------------------------------------------------------- #
#
# Several models, or several initial states, forecast from the same dates: `stack_forecasts` puts their records along a new dim
# 'member'.  For the members x_1..x_M of an element and its verification y:
#   mean x-bar;  spread sqrt(sum (x_i - x-bar)^2 / (M - ddof));
#   crps = A - B / 2,  A = (1 / M) sum_i |x_i - y|,  B = sum_ij |x_i - x_j| / M^2   (fair: / (M (M - 1)));
#   rank = the number of members strictly below y, 0..M.
# An element with a NaN or infinite member is missing (NaN, rank -1) everywhere, one with a NaN or infinite verification in crps
# and rank; the means over `axis` leave missing elements out.  numpy inputs take the host path (np.sort in float64), device
# tensors dlwpcs_ensemble_stats and then the score reduction; neither path falls back to the other.

_ENS_METHODS = ('crps', 'fair_crps', 'spread', 'ens_mse', 'ens_rmse', 'ssr')


def stack_forecasts(forecasts, dim='member'):
    """
    Stack forecast records of equal dims and coordinates along a new leading dim `dim` with the coordinate arange(M).

    :param forecasts: sequence of Forecast records (or of plain arrays / tensors of one shape)
    :param dim: name of the new dim
    :return: Forecast (plain array for plain inputs); device values stay on the device
    """
    recs = list(forecasts)
    if not recs:
        raise ValueError('stack_forecasts: nothing to stack')
    labelled = [hasattr(r, 'dims') for r in recs]
    if any(labelled) and not all(labelled):
        raise ValueError('stack_forecasts: labelled and plain records cannot be mixed')
    first = recs[0]
    for r in recs[1:]:
        _check_labels(first, r)
        if labelled[0] and set(getattr(first, 'coords', {})) != set(getattr(r, 'coords', {})):
            raise ValueError('stack_forecasts: the records carry different coordinates')
        if tuple(r.shape) != tuple(first.shape):
            raise ValueError('stack_forecasts: shapes %s and %s differ' % (tuple(first.shape), tuple(r.shape)))
    if labelled[0] and dim in first.dims:
        raise ValueError("stack_forecasts: the records already have a dim '%s'" % dim)
    vals = [_raw(r) for r in recs]
    if any(_is_tensor(v) for v in vals):
        import torch
        dev = next(v.device for v in vals if _is_tensor(v))
        stacked = torch.stack([v if _is_tensor(v) else torch.from_numpy(np.asarray(v)).to(dev) for v in vals])
    else:
        stacked = np.stack([np.asarray(v) for v in vals])
    if not labelled[0]:
        return stacked
    coords = dict(first.coords)
    coords[dim] = np.arange(len(recs))
    out = Forecast(stacked, (dim,) + tuple(first.dims), coords, name=getattr(first, 'name', 'forecast'))
    if hasattr(first, 'lat'):
        out.lat = first.lat
    return out


def _member_axis(ens, member_axis):
    """the member axis: the dim named 'member' of a labelled input, else `member_axis`"""
    nd = len(ens.shape)
    if hasattr(ens, 'dims'):
        if 'member' not in tuple(ens.dims):
            raise ValueError("the ensemble's dims %s have no 'member'" % (tuple(ens.dims),))
        return tuple(ens.dims).index('member')
    a = int(member_axis)
    if a < -nd or a >= nd:
        raise ValueError('member_axis %d out of range of %d axes' % (a, nd))
    return a % nd


def _check_ensemble(ens, valid, ax, min_members=2):
    """M; the verification must carry the ensemble's dims without the member dim (extents of 1 broadcast)"""
    M = int(ens.shape[ax])
    if M < min_members:
        raise ValueError('an ensemble needs at least %d members, got %d' % (min_members, M))
    if valid is None:
        return M
    eshape = tuple(int(e) for i, e in enumerate(ens.shape) if i != ax)
    vshape = tuple(int(e) for e in valid.shape)
    if len(vshape) == len(eshape) - 1:
        raise NotImplementedError('the lagged form against a continuous verification series (valid[f + t]) is not served: '
                                  'aligned arrays are')
    if hasattr(ens, 'dims') and hasattr(valid, 'dims'):
        ed, vd = tuple(d for d in ens.dims if d != 'member'), tuple(valid.dims)
        if ed != vd:
            raise ValueError('the ensemble dims %s without the member dim do not match the verification dims %s' % (ens.dims, vd))
        ec, vc = getattr(ens, 'coords', {}), getattr(valid, 'coords', {})
        for d, e, v in zip(ed, eshape, vshape):
            if d in ec and d in vc and v != 1:
                a, b = np.asarray(getattr(ec[d], 'values', ec[d])), np.asarray(getattr(vc[d], 'values', vc[d]))
                if a.shape != b.shape or not np.array_equal(a, b):
                    raise ValueError("coordinate '%s' of the ensemble and the verification differ (no alignment is done)" % d)
    if len(vshape) != len(eshape) or any(v not in (1, e) for v, e in zip(vshape, eshape)):
        raise ValueError('the verification %s must carry the dims of the ensemble without the member dim %s (extents of 1 '
                         'broadcast)' % (vshape, eshape))
    return M


def _ensemble_host(x, y, ax, want, fair, ddof, variance):
    """numpy twin of dlwpcs_ensemble_stats in float64: dict of the fields in `want`"""
    x = np.moveaxis(np.asarray(x, dtype=np.float64), ax, 0)
    M = x.shape[0]
    bad = ~np.isfinite(x).all(axis=0)
    xs = np.sort(np.where(bad, 0.0, x), axis=0)
    out = {}
    if 'mean' in want:
        out['mean'] = np.where(bad, np.nan, xs.mean(axis=0))
    if 'spread' in want:
        var = xs.var(axis=0, ddof=ddof)
        out['spread'] = np.where(bad, np.nan, var if variance else np.sqrt(var))
    if 'crps' in want or 'rank' in want:
        y = np.broadcast_to(np.asarray(y, dtype=np.float64), x.shape[1:])
        miss = bad | ~np.isfinite(y)
        y0 = np.where(miss, 0.0, y)
        if 'crps' in want:
            coef = (2.0 * np.arange(1, M + 1) - M - 1).reshape((M,) + (1,) * (x.ndim - 1))
            a = np.abs(xs - y0).mean(axis=0)
            b = 2.0 * (coef * xs).sum(axis=0) / (M * (M - 1) if fair else M * M)
            out['crps'] = np.where(miss, np.nan, a - b / 2.0)
        if 'rank' in want:
            out['rank'] = np.where(miss, -1, (xs < y0).sum(axis=0)).astype(np.int32)
    return out


def _ensemble_fields(ens, valid, ax, want, fair=False, ddof=1, variance=False):
    """the per-element fields in `want`: float64 / int32 numpy on the host path, device tensors on the device path"""
    if not _on_device(ens, valid):
        return _ensemble_host(_host(ens), None if valid is None else _host(valid), ax, want, fair, ddof, variance)
    import torch
    from . import ops as dops
    dev = next(_raw(x).device for x in (ens, valid) if x is not None and _is_tensor(_raw(x)) and _raw(x).is_cuda)
    with torch.cuda.device(dev):
        et = _dev_operand(ens, dev)
        vt = _dev_operand(valid, dev) if valid is not None else None
        return dops.ensemble_stats(et, vt, member_axis=ax, want=want, fair=fair, ddof=ddof, variance=variance)


def _ensemble_label(values, ens, extra_dim=None, name='ensemble', drop=()):
    """`values` labelled with the dims of `ens` without the member dim (and without the dims at the element positions `drop`)"""
    if not hasattr(ens, 'dims'):
        return values
    dims = tuple(d for d in ens.dims if d != 'member')
    dims = tuple(d for i, d in enumerate(dims) if i not in drop)
    coords = {d: np.asarray(getattr(ens.coords[d], 'values', ens.coords[d])) for d in dims if d in getattr(ens, 'coords', {})}
    if extra_dim is not None:
        dims = dims + (extra_dim,)
        coords[extra_dim] = np.arange(values.shape[-1])
    return Forecast(values, dims, coords, name=name)


def ensemble_mean(ens, member_axis=0):
    """
    The mean over the members of every element.

    :param ens: ensemble: ndarray, device tensor, or a labelled array with a dim 'member' (`stack_forecasts`)
    :param member_axis: the member axis of an unlabelled input
    :return: the field without the member dim, labelled like the input, on the device when the input is; NaN where a member is
        NaN or infinite
    """
    ax = _member_axis(ens, member_axis)
    _check_ensemble(ens, None, ax)
    return _ensemble_label(_ensemble_fields(ens, None, ax, ('mean',))['mean'], ens, name='ensemble_mean')


def ensemble_spread(ens, ddof=1, member_axis=0):
    """The standard deviation over the members of every element, sqrt(sum (x_i - mean)^2 / (M - ddof)); see `ensemble_mean`."""
    ax = _member_axis(ens, member_axis)
    _check_ensemble(ens, None, ax)
    return _ensemble_label(_ensemble_fields(ens, None, ax, ('spread',), ddof=ddof)['spread'], ens, name='ensemble_spread')


def ensemble_crps(ens, valid, fair=False, member_axis=0):
    """
    The continuous ranked probability score of every element, mean_i |x_i - y| - sum_ij |x_i - x_j| / (2 M^2); fair=True divides
    the pair term by M (M - 1) instead (the score of the distribution the members were drawn from rather than of the M-member
    step function).  `valid` carries the dims of `ens` without the member dim (extents of 1 broadcast); a continuous series
    with one axis fewer raises NotImplementedError.  NaN where a member or the verification is NaN or infinite.
    """
    ax = _member_axis(ens, member_axis)
    _check_ensemble(ens, valid, ax)
    return _ensemble_label(_ensemble_fields(ens, valid, ax, ('crps',), fair=fair)['crps'], ens, name='ensemble_crps')


def _field_mean(field, w, ax):
    """float64 nan-mean of field * w over the axes `ax` (numpy on the host, the score reduction on the device)"""
    if not _is_tensor(field):
        with np.errstate(invalid='ignore'):
            return np.asarray(_nanmean(field * (1. if w is None else w), ax), dtype=np.float64)
    import torch
    from . import ops as dops
    with torch.cuda.device(field.device):
        if w is not None:
            field = field * _dev_operand(w, field.device)
        shape = tuple(int(e) for e in field.shape)
        out = dops.score_reduce('mean', [None, (field, _bstrides(field, shape)), None, None], shape, set(ax))
        return np.asarray(out.cpu().numpy(), dtype=np.float64)


def _mean_error(mean, valid, method, w, ax):
    """forecast_error's aligned form on the ensemble mean: the same code on either path"""
    if not _is_tensor(mean):
        return np.asarray(_score_host(method, mean, _host(valid), 0., 1. if w is None else w, ax), dtype=np.float64)
    import torch
    dev = mean.device
    with torch.cuda.device(dev):
        wt = _dev_operand(w, dev) if w is not None else None
        return np.asarray(_aligned_device(method, mean, _dev_operand(valid, dev), None, wt, ax), dtype=np.float64)


def ensemble_error(ens, valid, method='crps', axis=None, weighted=False, member_axis=0):
    """
    A score of an ensemble forecast, averaged like `forecast_error`: `axis` counts the dims of the ensemble WITHOUT the member
    dim (None: every one but the first, the forecast hour), the mean over `axis` leaves missing elements out, the result is
    float64 with the forecast hour first.

    :param ens: ensemble (dim 'member' of a labelled input, else `member_axis`)
    :param valid: verification with the dims of `ens` without the member dim (extents of 1 broadcast)
    :param method: 'crps' / 'fair_crps': mean(crps w);  'spread': sqrt(mean(variance w)), the RMS spread (ddof = 1);
        'ens_mse' / 'ens_rmse': `forecast_error` of the ensemble mean;  'ssr': sqrt((M + 1) / M) spread / ens_rmse, near 1
        for an ensemble whose members are drawn from the distribution of the verification
    :param weighted: weight by cos(latitude) / its mean, read from `valid.lat`
    """
    if method not in _ENS_METHODS:
        raise ValueError("'method' must be one of %s" % ', '.join(repr(m) for m in _ENS_METHODS))
    mx = _member_axis(ens, member_axis)
    M = _check_ensemble(ens, valid, mx)
    nd = len(ens.shape) - 1
    ax = tuple(range(1, nd)) if axis is None else _axes(axis, nd)
    w = _weights(valid) if weighted else None
    if method in ('crps', 'fair_crps'):
        f = _ensemble_fields(ens, valid, mx, ('crps',), fair=method == 'fair_crps')
        return _field_mean(f['crps'], w, ax)
    want = {'spread': ('spread',), 'ssr': ('mean', 'spread')}.get(method, ('mean',))
    f = _ensemble_fields(ens, None, mx, want, ddof=1, variance=True)
    if method == 'spread':
        return np.sqrt(_field_mean(f['spread'], w, ax))
    if method in ('ens_mse', 'ens_rmse'):
        return _mean_error(f['mean'], valid, method[4:], w, ax)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.sqrt((M + 1.0) / M) * np.sqrt(_field_mean(f['spread'], w, ax)) / _mean_error(f['mean'], valid, 'rmse', w, ax)


def rank_histogram(ens, valid, axis=None, member_axis=0):
    """
    The rank histogram (Talagrand diagram): how often the verification has 0, 1, .. M members strictly below it, counted over
    `axis` (dims of the ensemble without the member dim; None: all of them).  Missing elements (rank -1) are left out.

    :return: exact int64 counts (kept axes..., M + 1), labelled like the input with a last dim 'rank'
    """
    mx = _member_axis(ens, member_axis)
    M = _check_ensemble(ens, valid, mx)
    nd = len(ens.shape) - 1
    ax = tuple(range(nd)) if axis is None else _axes(axis, nd)
    rank = _ensemble_fields(ens, valid, mx, ('rank',))['rank']
    kept = [i for i in range(nd) if i not in ax]
    kshape = [int(rank.shape[i]) for i in kept]
    K = int(np.prod(kshape)) if kept else 1
    if _is_tensor(rank):
        import torch
        r = rank.permute(kept + list(ax)).reshape(K, -1).to(torch.int64)
        idx = r + torch.arange(K, device=r.device, dtype=torch.int64)[:, None] * (M + 1)
        counts = torch.bincount(idx[r >= 0], minlength=K * (M + 1)).cpu().numpy()
    else:
        r = np.transpose(rank, kept + list(ax)).reshape(K, -1).astype(np.int64)
        idx = r + np.arange(K, dtype=np.int64)[:, None] * (M + 1)
        counts = np.bincount(idx[r >= 0], minlength=K * (M + 1))
    counts = np.asarray(counts, dtype=np.int64).reshape(kshape + [M + 1])
    return _ensemble_label(counts, ens, extra_dim='rank', name='rank_histogram', drop=ax)


# --------------------------------------------------------------------------------------------------------------------- #
# Categorical probability scores of an ensemble
# --------------------------------------------------------------------------------------------------------------------- #
#
# Against Q thresholds t_0 <= .. <= t_{Q-1} per element -- climatological terciles from `climatology_quantiles`, or fixed values --
# with k_j = #{i : x_i <= t_j} of the M members and o_j = 1{y <= t_j} of the verification:
#   probability p_j = k_j / M;   brier_j = (p_j - o_j)^2;   rps = sum_j brier_j   (fair: minus sum_j k_j (M - k_j) / (M^2 (M - 1)));
#   the reference forecast's rps_ref = sum_j (P_j - o_j)^2 with the climatological probabilities P_j, e.g. (1/3, 2/3);
#   rpss = 1 - mean(rps) / mean(rps_ref);   code_j = 2 k_j + o_j, what `reliability_counts` counts.
# Missing elements (a NaN or infinite member or verification, a NaN threshold) are NaN / -1 and left out of every mean and count.
# numpy inputs take the host path in float64, device tensors dlwpcs_ensemble_category (float32, each operation rounded once) and
# then the score reduction; neither path falls back to the other.

_CAT_METHODS = ('brier', 'rps', 'fair_rps', 'rpss', 'fair_rpss')
_THRESHOLD_DIMS = ('quantile', 'threshold')


def _threshold_operand(ens, thresholds, mx, threshold_axis):
    """(thresholds, their threshold axis, Q, dim name, coordinate or None): the threshold dim is 'quantile' or 'threshold' of a
    labelled input, else `threshold_axis`; the other dims must be those of the ensemble without the member dim (extents of 1
    broadcast), or there are none (a bare vector).  A ClimatologyLookup is laid out first."""
    if isinstance(thresholds, ClimatologyLookup):
        thresholds = thresholds.materialize()
    if not hasattr(thresholds, 'shape'):
        thresholds = np.asarray(thresholds, dtype=np.float64)
    shape = tuple(int(e) for e in thresholds.shape)
    name, coord = 'threshold', None
    if len(shape) < 1:
        raise ValueError('the thresholds need a threshold axis')
    if hasattr(thresholds, 'dims'):
        td = tuple(thresholds.dims)
        found = [d for d in _THRESHOLD_DIMS if d in td]
        if len(found) != 1:
            raise ValueError("the thresholds' dims %s must hold one of 'quantile' and 'threshold'" % (td,))
        name = found[0]
        ta = td.index(name)
        if name in getattr(thresholds, 'coords', {}):
            coord = _coord(thresholds, name)
        if hasattr(ens, 'dims') and len(td) > 1:
            ed = tuple(d for d in ens.dims if d != 'member')
            if td[:ta] + td[ta + 1:] != ed:
                raise ValueError("the thresholds' dims %s without '%s' do not match the ensemble dims %s without the member dim"
                                 % (td, name, tuple(ens.dims)))
    else:
        a = int(threshold_axis)
        if a < -len(shape) or a >= len(shape):
            raise ValueError('threshold_axis %d out of range of %d axes' % (a, len(shape)))
        ta = a % len(shape)
    eshape = tuple(int(e) for i, e in enumerate(ens.shape) if i != mx)
    if len(shape) > 1:
        rest = shape[:ta] + shape[ta + 1:]
        if len(rest) != len(eshape) or any(t not in (1, e) for t, e in zip(rest, eshape)):
            raise ValueError('the thresholds %s without their threshold axis must carry the dims of the ensemble without the '
                             'member dim %s (extents of 1 broadcast)' % (shape, eshape))
    if shape[ta] < 1:
        raise ValueError('at least one threshold is needed')
    return thresholds, ta, shape[ta], name, coord


def _category_host(x, y, t, ax, ta, want, fair, ref_prob):
    """numpy twin of dlwpcs_ensemble_category in float64: dict of the fields in `want` (threshold first where there is one)"""
    x = np.moveaxis(np.asarray(x, dtype=np.float64), ax, 0)
    M, eshape = x.shape[0], x.shape[1:]
    t = np.asarray(t, dtype=np.float64)
    t = np.moveaxis(t, ta, 0) if t.ndim > 1 else t.reshape((-1,) + (1,) * len(eshape))
    Q = t.shape[0]
    bad = ~np.isfinite(x).all(axis=0)
    out = {}
    with np.errstate(invalid='ignore'):
        k = np.stack([(x <= t[j]).sum(axis=0) for j in range(Q)]).astype(np.int64)
        tnan = np.broadcast_to(np.isnan(t), k.shape)
        miss = bad[None] | tnan
        if 'prob' in want:
            out['prob'] = np.where(miss, np.nan, k / float(M))
        if want != ('prob',):
            y = np.broadcast_to(np.asarray(y, dtype=np.float64), eshape)
            ymiss = miss | ~np.isfinite(y)[None]
            o = (y[None] <= np.broadcast_to(t, k.shape)).astype(np.int64)
            brier = ((k - o * M) / float(M)) ** 2
            whole = ymiss.any(axis=0)
            if 'brier' in want:
                out['brier'] = np.where(ymiss, np.nan, brier)
            if 'rps' in want:
                rps = brier.sum(axis=0)
                if fair:
                    rps = rps - (k * (M - k)).sum(axis=0) / (float(M) * M * (M - 1))
                out['rps'] = np.where(whole, np.nan, rps)
            if 'rps_ref' in want:
                P = np.asarray(ref_prob, dtype=np.float64).reshape((Q,) + (1,) * len(eshape))
                out['rps_ref'] = np.where(whole, np.nan, ((P - o) ** 2).sum(axis=0))
            if 'code' in want:
                out['code'] = np.where(ymiss, -1, 2 * k + o).astype(np.int32)
    return out


def _category_fields(ens, valid, thresholds, mx, ta, want, fair=False, ref_prob=None):
    """the per-element fields in `want`: float64 / int32 numpy on the host path, device tensors on the device path"""
    if ref_prob is not None:
        ref_prob = np.asarray(ref_prob, dtype=np.float64).reshape(-1)
    if not _on_device(ens, valid, thresholds):
        return _category_host(_host(ens), None if valid is None else _host(valid), _host(thresholds), mx, ta, want, fair, ref_prob)
    import torch
    from . import ops as dops
    dev = next(_raw(x).device for x in (ens, valid, thresholds) if x is not None and _is_tensor(_raw(x)) and _raw(x).is_cuda)
    with torch.cuda.device(dev):
        et, tt = _dev_operand(ens, dev), _dev_operand(thresholds, dev)
        vt = _dev_operand(valid, dev) if valid is not None else None
        return dops.ensemble_category(et, vt, tt, member_axis=mx, threshold_axis=ta, want=want, fair=fair, ref_prob=ref_prob)


def _category_label(values, ens, lead=(), tail=(), name='category', drop=()):
    """`values` labelled with the dims of `ens` without the member dim (and without the element positions `drop`), behind the
    dims `lead` and in front of the dims `tail`: sequences of (name, coordinate)"""
    if not hasattr(ens, 'dims'):
        return values
    dims = tuple(d for d in ens.dims if d != 'member')
    dims = tuple(d for i, d in enumerate(dims) if i not in drop)
    coords = {d: np.asarray(getattr(ens.coords[d], 'values', ens.coords[d])) for d in dims if d in getattr(ens, 'coords', {})}
    for n, c in tuple(lead) + tuple(tail):
        coords[n] = np.asarray(c)
    out = Forecast(values, tuple(n for n, _ in lead) + dims + tuple(n for n, _ in tail), coords, name=name)
    if hasattr(ens, 'lat'):
        out.lat = ens.lat
    return out


def ensemble_probability(ens, thresholds, member_axis=0, threshold_axis=0):
    """
    The forecast probability of every category boundary: the share of the members at or below each threshold, P(x <= t_j).

    :param ens: ensemble: ndarray, device tensor, or a labelled array with a dim 'member' (`stack_forecasts`)
    :param thresholds: Q <= 16 thresholds per element: an array with the dims of `ens` without the member dim (extents of 1
        broadcast) and a threshold dim -- the dim 'quantile' or 'threshold' of a labelled input (`climatology_quantiles`,
        `daily_climo_time_series` of it, also lazy), else `threshold_axis` -- or a bare (Q,) vector for every element
    :return: the (Q, ...) field, threshold first, labelled like the input, on the device when an input is; NaN where a member
        is NaN or infinite or the threshold is NaN
    """
    mx = _member_axis(ens, member_axis)
    _check_ensemble(ens, None, mx, 1)
    thr, ta, Q, tname, tcoord = _threshold_operand(ens, thresholds, mx, threshold_axis)
    f = _category_fields(ens, None, thr, mx, ta, ('prob',))['prob']
    return _category_label(f, ens, lead=[(tname, np.arange(Q) if tcoord is None else tcoord)], name='ensemble_probability')


def brier_score(ens, valid, thresholds, member_axis=0, threshold_axis=0):
    """
    The Brier score of every element and threshold, (k_j / M - 1{y <= t_j})^2 with k_j the members at or below t_j; operands
    as in `ensemble_probability`, `valid` as in `ensemble_crps` (a continuous series with one axis fewer raises
    NotImplementedError).  Returns the (Q, ...) field; NaN where a member, the verification or the threshold is missing.
    """
    mx = _member_axis(ens, member_axis)
    _check_ensemble(ens, valid, mx, 1)
    thr, ta, Q, tname, tcoord = _threshold_operand(ens, thresholds, mx, threshold_axis)
    f = _category_fields(ens, valid, thr, mx, ta, ('brier',))['brier']
    return _category_label(f, ens, lead=[(tname, np.arange(Q) if tcoord is None else tcoord)], name='brier_score')


def ranked_probability_score(ens, valid, thresholds, fair=False, member_axis=0, threshold_axis=0):
    """
    The ranked probability score of every element: the sum of the Brier scores over the Q thresholds (the Q + 1 categories they
    bound).  fair=True subtracts sum_j k_j (M - k_j) / (M^2 (M - 1)): the score an ensemble of infinitely many members drawn
    like these would get in expectation (needs 2 members).  Operands as in `brier_score`; returns the (...) field.
    """
    mx = _member_axis(ens, member_axis)
    _check_ensemble(ens, valid, mx, 2 if fair else 1)
    thr, ta, _, _, _ = _threshold_operand(ens, thresholds, mx, threshold_axis)
    f = _category_fields(ens, valid, thr, mx, ta, ('rps',), fair=fair)['rps']
    return _category_label(f, ens, name='ranked_probability_score')


def categorical_error(ens, valid, thresholds, method='rps', axis=None, weighted=False, probabilities=None, member_axis=0,
                      threshold_axis=0):
    """
    A categorical score of an ensemble forecast, averaged like `ensemble_error`: `axis` counts the dims of the ensemble WITHOUT
    the member dim (None: every one but the first, the forecast hour), the mean over `axis` leaves missing elements out, the
    result is float64 with the forecast hour first.

    :param thresholds: as in `ensemble_probability`
    :param method: 'brier': mean(brier w), with a last axis of Q;  'rps' / 'fair_rps': mean(rps w);  'rpss' / 'fair_rpss':
        1 - mean(rps w) / mean(rps_ref w), the skill against the reference forecast that issues `probabilities` every time --
        with one threshold this is the Brier skill score
    :param probabilities: the Q climatological probabilities P(y <= t_j) of the reference forecast, (1 / 3, 2 / 3) for
        terciles; needed by 'rpss' and 'fair_rpss'
    :param weighted: weight by cos(latitude) / its mean, read from `valid.lat`
    """
    if method not in _CAT_METHODS:
        raise ValueError("'method' must be one of %s" % ', '.join(repr(m) for m in _CAT_METHODS))
    fair, skill = method.startswith('fair_'), method.endswith('rpss')
    mx = _member_axis(ens, member_axis)
    _check_ensemble(ens, valid, mx, 2 if fair else 1)
    thr, ta, Q, _, _ = _threshold_operand(ens, thresholds, mx, threshold_axis)
    ref = None
    if skill:
        if probabilities is None:
            raise ValueError("'%s' needs the reference forecast's `probabilities`, e.g. (1 / 3, 2 / 3)" % method)
        ref = np.asarray(probabilities, dtype=np.float64).reshape(-1)
        if ref.size != Q or not np.all((ref >= 0.) & (ref <= 1.)):
            raise ValueError('`probabilities` must be %d values in [0, 1], got %s' % (Q, ref))
    nd = len(ens.shape) - 1
    ax = tuple(range(1, nd)) if axis is None else _axes(axis, nd)
    w = _weights(valid) if weighted else None
    if method == 'brier':
        f = _category_fields(ens, valid, thr, mx, ta, ('brier',))['brier']
        return np.stack([_field_mean(f[j], w, ax) for j in range(Q)], axis=-1)
    f = _category_fields(ens, valid, thr, mx, ta, ('rps', 'rps_ref') if skill else ('rps',), fair=fair, ref_prob=ref)
    score = _field_mean(f['rps'], w, ax)
    if not skill:
        return score
    with np.errstate(invalid='ignore', divide='ignore'):
        return 1.0 - score / _field_mean(f['rps_ref'], w, ax)


def reliability_counts(ens, valid, thresholds, axis=None, member_axis=0, threshold_axis=0):
    """
    The joint counts of forecast probability and outcome that reliability diagrams and ROC curves are drawn from: per threshold
    j, how often k of the M members lay at or below it (the forecast probability k / M of the event y <= t_j) while the event
    did (observed = 1) or did not (0) happen, counted over `axis` (dims of the ensemble without the member dim; None: all of
    them).  Missing elements are left out.

    With c = counts[..., j, :, :]: the reliability curve plots the observed frequency c[k, 1] / (c[k, 0] + c[k, 1]) against the
    forecast probability k / M, with c[k, 0] + c[k, 1] the sharpness histogram; the ROC point of the rule "warn when at least m
    members are at or below the threshold" has the hit rate c[m:, 1].sum() / c[:, 1].sum() and the false alarm rate
    c[m:, 0].sum() / c[:, 0].sum().

    :return: exact int64 counts (kept axes..., Q, M + 1, 2), labelled like the input with the last dims ('threshold',
        'members_below', 'observed')
    """
    mx = _member_axis(ens, member_axis)
    M = _check_ensemble(ens, valid, mx, 1)
    thr, ta, Q, _, tcoord = _threshold_operand(ens, thresholds, mx, threshold_axis)
    nd = len(ens.shape) - 1
    ax = tuple(range(nd)) if axis is None else _axes(axis, nd)
    code = _category_fields(ens, valid, thr, mx, ta, ('code',))['code']
    kept = [i for i in range(nd) if i not in ax]
    kshape = [int(code.shape[1 + i]) for i in kept]
    K = (int(np.prod(kshape)) if kept else 1) * Q
    width = 2 * (M + 1)
    order = [1 + i for i in kept] + [0] + [1 + i for i in ax]
    if _is_tensor(code):
        import torch
        c = code.permute(order).reshape(K, -1).to(torch.int64)
        idx = c + torch.arange(K, device=c.device, dtype=torch.int64)[:, None] * width
        counts = torch.bincount(idx[c >= 0], minlength=K * width).cpu().numpy()
    else:
        c = np.transpose(code, order).reshape(K, -1).astype(np.int64)
        idx = c + np.arange(K, dtype=np.int64)[:, None] * width
        counts = np.bincount(idx[c >= 0], minlength=K * width)
    counts = np.asarray(counts, dtype=np.int64).reshape(kshape + [Q, M + 1, 2])
    tail = [('threshold', np.arange(Q) if tcoord is None else tcoord), ('members_below', np.arange(M + 1)), ('observed', np.arange(2))]
    return _category_label(counts, ens, tail=tail, name='reliability_counts', drop=ax)


# --------------------------------------------------------------------------------------------------------------------- #
# Filters along time: running means, Lanczos low-pass and band-pass (the reference leaves xarray's rolling().mean() to the user)
# --------------------------------------------------------------------------------------------------------------------- #

_FILTER_LABELS = ('end', 'centre', 'start')


def lanczos_weights(n, cutoff, cutoff_high=None):
    """
    The 2 n + 1 taps of a Lanczos low-pass filter with the cut-off frequency `cutoff` in cycles per row (Duchon 1979):
    w_k = 2 fc sinc(2 fc k) sinc(k / (n + 1)) for k = -n .. n with sinc(x) = sin(pi x) / (pi x), normalised to sum 1.  With
    `cutoff_high` the band-pass low(cutoff_high) - low(cutoff), which sums to 0: it keeps the periods between 1 / cutoff_high
    and 1 / cutoff rows (2 to 6 days of 6-hourly data: cutoff = 1 / 24, cutoff_high = 1 / 8).  float64, symmetric to the last
    bit.  Host only.
    """
    n = int(n)
    if n < 1:
        raise ValueError('lanczos_weights: n must be at least 1, got %d' % n)
    for fc in (cutoff,) if cutoff_high is None else (cutoff, cutoff_high):
        if not 0. < float(fc) <= 0.5:
            raise ValueError('lanczos_weights: a cut-off of %r cycles per row is outside (0, 0.5]' % (fc,))
    if cutoff_high is not None and not float(cutoff_high) > float(cutoff):
        raise ValueError('lanczos_weights: cutoff_high must lie above cutoff')

    def low(fc):
        k = np.arange(1, n + 1, dtype=np.float64)
        half = 2. * fc * np.sinc(2. * fc * k) * np.sinc(k / (n + 1.))
        w = np.concatenate([half[::-1], [2. * fc], half])
        return w / (2. * fc + 2. * half.sum())

    w = low(float(cutoff))
    if cutoff_high is None:
        return w
    b = low(float(cutoff_high)) - w
    # the two halves are the same numbers in mirrored order, so the sum below is the only thing left to centre
    b[n] -= b.sum()
    return b


def _filter_axis(x, axis, name):
    dims = tuple(getattr(x, 'dims', ()))
    nd = len(_raw(x).shape)
    if axis is None:
        return dims.index(name) if name in dims else 0
    if isinstance(axis, str):
        if axis not in dims:
            raise ValueError("the data has no '%s' dimension (dims: %s)" % (axis, ', '.join(dims)))
        return dims.index(axis)
    if not -nd <= int(axis) < nd:
        raise ValueError('axis %d is out of range of %d dims' % (axis, nd))
    return int(axis) % nd


def _fp32_sum(h32):
    s = np.float32(0.)
    for v in h32:
        s = np.float32(s + v)
    return s


def _time_filter_host(x, h, axis, step, origin, n_out, mean, threshold):
    """the definition of dlwpcs_time_filter in float64: (values, int32 counts)"""
    v = np.moveaxis(np.asarray(x, dtype=np.float64), axis, 0)
    T, K = v.shape[0], len(h)
    acc = np.zeros((n_out,) + v.shape[1:], dtype=np.float64)
    w = np.zeros_like(acc)
    n = np.zeros(acc.shape, dtype=np.int32)
    j = np.arange(n_out, dtype=np.int64)
    tail = (slice(None),) + (None,) * (v.ndim - 1)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        for k in range(K):
            r = j * step + k - origin
            inside = (r >= 0) & (r < T)
            rows = v[np.clip(r, 0, max(T - 1, 0))] if T else np.full(acc.shape, np.nan)
            present = inside[tail] & ~np.isnan(rows)
            acc = acc + np.where(present, h[k] * np.where(present, rows, 0.), 0.)
            w = w + np.where(present, h[k], 0.)
            n += present
        if mean:
            q = acc / w
            out = np.where((n > 0) & (w >= threshold) & ~np.isnan(q), q, np.nan)
        else:
            out = np.where((n == K) & ~np.isnan(acc), acc, np.nan)
    return np.moveaxis(out, 0, axis), np.moveaxis(n, 0, axis)


def _filter_label(x, axis, rows, values, name):
    """`values` labelled like x, the coordinate of `axis` taken at the source rows `rows`"""
    if not hasattr(x, 'dims'):
        return values
    dims = tuple(x.dims)
    coords = {}
    for i, d in enumerate(dims):
        if d in getattr(x, 'coords', {}):
            c = _coord(x, d)
            coords[d] = c[rows] if i == axis else c
    out = Forecast(values, dims, coords, name=name)
    if hasattr(x, 'lat'):
        out.lat = x.lat
    return out


def _time_filter_apply(x, h, axis, step, mode, mean, min_weight, relative, label, return_count, name):
    if mode not in ('valid', 'same'):
        raise ValueError("'mode' must be 'valid' or 'same'")
    if label is None:
        label = 'end' if mode == 'valid' else 'centre'
    if label not in _FILTER_LABELS:
        raise ValueError("'label' must be 'end', 'centre' or 'start'")
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    K, step = int(h.size), int(step)
    if K < 1:
        raise ValueError('%s: no weights' % name)
    if step < 1:
        raise ValueError('%s: step must be at least 1, got %d' % (name, step))
    if not np.all(np.isfinite(h)):
        raise ValueError('%s: the weights must be finite' % name)
    if mean and not (np.all(h >= 0.) and h.sum() > 0.):
        raise ValueError("%s: skipping missing values needs weights >= 0 with a positive sum" % name)
    v = _raw(x)
    T = int(v.shape[axis])
    if mode == 'valid':
        origin, J = 0, max(0, (T - K) // step + 1)
    else:
        origin, J = (K - 1) // 2, -(-T // step)
    first = np.arange(J, dtype=np.int64) * step - origin
    rows = first + {'end': K - 1, 'centre': (K - 1) // 2, 'start': 0}[label]
    if hasattr(x, 'dims') and J and (rows[0] < 0 or rows[-1] >= T):
        raise ValueError("%s: label='%s' lies outside the series in mode '%s'" % (name, label, mode))
    if _is_tensor(v) and v.is_cuda:
        import torch
        from . import ops as dops
        h32 = h.astype(np.float32)
        thr = np.float32(np.float32(min_weight) * _fp32_sum(h32)) if relative else np.float32(min_weight)
        with torch.cuda.device(v.device):
            src = v if v.dtype == torch.float32 else v.to(torch.float32)
            res = dops.time_filter(src, h, row_axis=axis, step=step, origin=origin, n_out=J, mode='mean' if mean else 'sum',
                                   min_weight=float(thr), counts=return_count)
        out, cnt = res if return_count else (res, None)
    else:
        tot = 0.
        for hk in h:
            tot = tot + hk
        thr = float(min_weight) * tot if relative else float(min_weight)
        out, cnt = _time_filter_host(_host(v), h, axis, step, origin, J, mean, thr)
    out = _filter_label(x, axis, rows, out, name)
    return (out, _filter_label(x, axis, rows, cnt, name + '_count')) if return_count else out


def time_filter(x, weights, axis=None, step=1, mode='valid', missing='propagate', min_weight=0.5, label=None, return_count=False):
    """
    Filter a series along time with the weights `weights` (K of them, at most 4096): output j is the sum over k of
    weights[k] * x[j * step + k - origin].

    :param x: a `Forecast` (or anything with `.dims`, `.coords`, `.values`), a numpy array or a torch tensor.  Values on a HIP
        device are filtered there (dlwpcs_time_filter: fp32, in tap order, one launch) and the result stays there; numpy values
        are filtered on the host in float64 by the same rules.
    :param weights: the taps, host values (e.g. `lanczos_weights`)
    :param axis: the axis to filter along, a position or a dim name; None: the 'time' dim of a labelled input, else axis 0
    :param step: keep every step-th output
    :param mode: 'valid': the windows that lie inside the series, origin 0, max(0, (T - K) // step + 1) outputs.  'same': the
        window is centred (origin (K - 1) // 2), ceil(T / step) outputs, the windows over the ends have missing entries
    :param missing: a NaN entry, or one outside the series, is missing.  'propagate': the output is NaN.  'skip': the weighted
        mean of the entries present (weights >= 0), NaN where their weight is below `min_weight` times the sum of the weights
    :param label: the time coordinate of an output is that of its window's 'end' (default for 'valid'), 'centre' (default for
        'same') or 'start'
    :param return_count: also return the int32 number of entries present in each window
    :return: labelled like the input (a plain array for a plain input)
    """
    if missing not in ('propagate', 'skip'):
        raise ValueError("'missing' must be 'propagate' or 'skip'")
    return _time_filter_apply(x, weights, _filter_axis(x, axis, 'time'), step, mode, missing == 'skip', min_weight, True, label, return_count,
                   'time_filter')


def running_mean(x, n, axis=None, step=1, mode='valid', min_count=None, label=None, return_count=False):
    """
    The mean over windows of `n` rows along time (`time_filter` with n weights of one): the sum of the entries present, in row
    order, over their exact count; NaN where fewer than `min_count` are present.  min_count=None: n, every entry present, the
    default of xarray's rolling().  The weekly mean of 6-hourly data is running_mean(x, 28), every day of it step=4.
    """
    n = int(n)
    if n < 1:
        raise ValueError('running_mean: a window of %d rows' % n)
    mc = n if min_count is None else int(min_count)
    if not 1 <= mc <= n:
        raise ValueError('running_mean: min_count %d outside 1 .. %d' % (mc, n))
    return _time_filter_apply(x, np.ones(n), _filter_axis(x, axis, 'time'), step, mode, True, mc, False, label, return_count, 'running_mean')


def lead_window_mean(x, windows, axis=None, min_count=None):
    """
    Means over unequal windows of the lead axis (week 3, week 4, weeks 5 to 6 of a forecast): window i holds the rows
    windows[i][0] .. windows[i][1] - 1.  NaN entries are skipped; a window with fewer than `min_count` entries present (None:
    its length) is NaN.  axis=None: the 'f_hour' dim of a labelled input, else axis 0.  The coordinate of a window is that of
    its last row.  Device values are reduced there (dlwpcs_group_mean, fp64 sums), numpy values on the host in fp64.
    """
    axis = _filter_axis(x, axis, 'f_hour')
    v = _raw(x)
    T = int(v.shape[axis])
    win = np.asarray(windows, dtype=np.int64).reshape(-1, 2)
    if win.shape[0] < 1 or np.any(win[:, 0] < 0) or np.any(win[:, 1] > T) or np.any(win[:, 1] <= win[:, 0]):
        raise ValueError('lead_window_mean: windows must be (start, stop) row pairs with 0 <= start < stop <= %d' % T)
    length = win[:, 1] - win[:, 0]
    mc = length if min_count is None else np.broadcast_to(np.asarray(min_count, dtype=np.int64), length.shape)
    if np.any(mc < 1) or np.any(mc > length):
        raise ValueError('lead_window_mean: min_count outside 1 .. the length of its window')
    start = np.concatenate([[0], np.cumsum(length)])
    order = np.concatenate([np.arange(a, b) for a, b in win])
    shape = [1] * len(v.shape)
    shape[axis] = len(mc)
    if _is_tensor(v) and v.is_cuda:
        import torch
        from . import ops as dops
        with torch.cuda.device(v.device):
            src = v if v.dtype == torch.float32 else v.to(torch.float32)
            out, cnt = dops.group_mean(src, start, order, row_axis=axis, counts=True)
            need = torch.from_numpy(np.ascontiguousarray(mc.reshape(shape), dtype=np.int32)).to(v.device)
            out = torch.where(cnt >= need, out, torch.full_like(out, float('nan')))
    else:
        h = np.moveaxis(np.asarray(_host(v), dtype=np.float64), axis, 0)
        out = np.empty((len(mc),) + h.shape[1:], dtype=np.float32)
        with np.errstate(invalid='ignore', divide='ignore'):
            for i, (a, b) in enumerate(win):
                ok = ~np.isnan(h[a:b])
                n = ok.sum(axis=0)
                out[i] = np.where(n >= mc[i], np.where(ok, h[a:b], 0.).sum(axis=0) / np.maximum(n, 1), np.nan)
        out = np.moveaxis(out, 0, axis)
    return _filter_label(x, axis, win[:, 1] - 1, out, 'lead_window_mean')


# --------------------------------------------------------------------------------------------------------------------- #
# Least-squares fits along time: trends, harmonic climatologies, regression maps
# --------------------------------------------------------------------------------------------------------------------- #

REGRESSION_MAX_TERMS = 16
_TROPICAL_YEAR_S = 365.24219 * 86400.
_FIT_SLAB = 512
_FIT_PIVOT_TOL = 2.0 ** -40


def _centred(t):
    """t mapped linearly onto [-1, 1] (one time: 0)"""
    t = np.asarray(t, dtype=np.float64)
    lo, hi = (t.min(), t.max()) if t.size else (0., 0.)
    return (2. * t - (hi + lo)) / (hi - lo) if hi > lo else np.zeros_like(t)


def _times_seconds(times):
    t = np.asarray(getattr(times, 'values', times))
    if t.dtype.kind == 'M':
        return (t.astype('datetime64[ms]') - np.datetime64('2000-01-01T00', 'ms')).astype(np.float64) / 1000., True
    return t.astype(np.float64), False


def harmonic_basis(times, n_harmonics=4, trend=False, period=None, trend_span=None):
    """
    The (T, K) float64 basis of a harmonic fit at `times`: a column of ones, with `trend` a linear trend centred and scaled to
    [-1, 1] over the times (over `trend_span` = (first, last) when given, so that other times continue the same line), then
    cos and sin of the harmonics 1 .. n_harmonics of `period`.  datetime64 times: the period is the tropical year (365.24219
    days) and the phase is counted from 2000-01-01; numbers: `period` must be given, in the unit of the times.  Host only.
    """
    t, is_date = _times_seconds(times)
    if t.ndim != 1:
        raise ValueError('harmonic_basis: the times must be one-dimensional')
    H = int(n_harmonics)
    if H < 0:
        raise ValueError('harmonic_basis: n_harmonics %d' % H)
    if period is None:
        if not is_date:
            raise ValueError('harmonic_basis: numeric times need a period')
        p = _TROPICAL_YEAR_S
    else:
        p = float(period / np.timedelta64(1, 's')) if isinstance(period, np.timedelta64) else float(period)
        if not p > 0.:
            raise ValueError('harmonic_basis: period %r' % (period,))
    cols = [np.ones(t.shape)]
    if trend:
        if trend_span is None:
            cols.append(_centred(t))
        else:
            lo, hi = _times_seconds(np.asarray(trend_span))[0]
            cols.append((2. * t - (hi + lo)) / (hi - lo) if hi > lo else np.zeros_like(t))
    for h in range(1, H + 1):
        ang = 2. * np.pi * h * (t / p)
        cols += [np.cos(ang), np.sin(ang)]
    if len(cols) > REGRESSION_MAX_TERMS:
        raise ValueError('harmonic_basis: %d terms (1 .. %d)' % (len(cols), REGRESSION_MAX_TERMS))
    return np.stack(cols, axis=1)


def _fit_basis32(basis, n_rows, name):
    """the basis as the device sees it: float32, checked"""
    b = np.asarray(getattr(basis, 'values', basis), dtype=np.float64)
    if b.ndim != 2:
        raise ValueError('%s: the basis must be (T, K), got %d dims' % (name, b.ndim))
    if not 1 <= b.shape[1] <= REGRESSION_MAX_TERMS:
        raise ValueError('%s: %d terms (1 .. %d)' % (name, b.shape[1], REGRESSION_MAX_TERMS))
    if n_rows is not None and b.shape[0] != n_rows:
        raise ValueError('%s: the basis has %d rows, the data %d' % (name, b.shape[0], n_rows))
    with np.errstate(over='ignore'):
        b32 = np.ascontiguousarray(b, dtype=np.float32)
    if not np.all(np.isfinite(b32)):
        raise ValueError('%s: the basis must be finite in float32' % name)
    return b32


def _time_regression_host(x, b32, axis, propagate, min_count):
    """the definition of dlwpcs_time_regression in float64 on the host: (float32 coefficients, int32 counts), the term axis where
    `axis` stood.  The same operations on the same rounded basis; the sums are numpy's, not the slab order: no claim to the bits."""
    v = np.moveaxis(np.asarray(x, dtype=np.float64), axis, 0)
    T, K = b32.shape
    rest = v.shape[1:]
    v = v.reshape(T, -1)
    E = v.shape[1]
    b = b32.astype(np.float64)
    present = ~np.isnan(v)
    n = present.sum(axis=0).astype(np.int32)
    with np.errstate(all='ignore'):
        xz = np.where(present, v, 0.)
        c = b.T @ xz                                                    # (K, E); an infinity stays one (0 * inf: NaN, as on the device)
        pm = present.astype(np.float64)
        G = np.zeros((K, K, E))
        for i in range(K):
            for j in range(i + 1):
                G[i, j] = (b[:, i] * b[:, j]) @ pm
        L, d = np.zeros((K, K, E)), np.zeros((K, E))
        singular = np.zeros(E, dtype=bool)
        for j in range(K):
            s = np.zeros(E)
            for p in range(j):
                s = s + (L[j, p] * L[j, p]) * d[p]
            dj = G[j, j] - s
            singular |= ~(dj > _FIT_PIVOT_TOL * G[j, j])
            d[j] = np.where(singular, np.nan, dj)
            for i in range(j + 1, K):
                s = np.zeros(E)
                for p in range(j):
                    s = s + (L[i, p] * L[j, p]) * d[p]
                L[i, j] = (G[i, j] - s) / d[j]
        z = np.zeros((K, E))
        for i in range(K):
            s = np.zeros(E)
            for p in range(i):
                s = s + L[i, p] * z[p]
            z[i] = c[i] - s
        w = z / d
        a = np.zeros((K, E))
        for i in range(K - 1, -1, -1):
            s = np.zeros(E)
            for p in range(i + 1, K):
                s = s + L[p, i] * a[p]
            a[i] = w[i] - s
        coef = a.astype(np.float32)
    bad = (n < min_count) | singular | ~np.all(np.isfinite(coef), axis=0)
    if propagate:
        bad |= n < T
    coef[:, bad] = np.nan
    return np.moveaxis(coef.reshape((K,) + rest), 0, axis), n.reshape(rest)


def _fit_label(x, axis, values, name, term=True):
    """`values` labelled like x with a 'term' dim where `axis` stood (term=False: without that dim)"""
    if not hasattr(x, 'dims'):
        return values
    dims = tuple(x.dims)
    coords = {d: _coord(x, d) for i, d in enumerate(dims) if i != axis and d in getattr(x, 'coords', {})}
    if term:
        coords['term'] = np.arange(values.shape[axis])
        out_dims = dims[:axis] + ('term',) + dims[axis + 1:]
    else:
        out_dims = dims[:axis] + dims[axis + 1:]
    out = Forecast(values, out_dims, coords, name=name)
    if hasattr(x, 'lat'):
        out.lat = x.lat
    return out


def _fit(x, b32, axis, missing, min_count, return_count, name):
    if missing not in ('propagate', 'skip'):
        raise ValueError("'missing' must be 'propagate' or 'skip'")
    K = b32.shape[1]
    mc = K if min_count is None else int(min_count)
    if mc < K:
        raise ValueError('%s: min_count %d below the %d terms' % (name, mc, K))
    v = _raw(x)
    if _is_tensor(v) and v.is_cuda:
        import torch
        from . import ops as dops
        with torch.cuda.device(v.device):
            src = v if v.dtype == torch.float32 else v.to(torch.float32)
            res = dops.time_regression(src, b32, row_axis=axis, missing=missing, min_count=mc, counts=return_count)
        coef, cnt = res if return_count else (res, None)
    else:
        coef, cnt = _time_regression_host(_host(v), b32, axis, missing == 'propagate', mc)
    out = _fit_label(x, axis, coef, name)
    return (out, _fit_label(x, axis, cnt, name + '_count', term=False)) if return_count else out


def time_regression(x, basis, axis=None, missing='skip', min_count=None, return_count=False):
    """
    The least-squares coefficients of `basis` (T, K; K at most 16) fitted along time, per grid point, to the rows that are not
    NaN: a trend, a harmonic climatology (`harmonic_basis`), or the regression of a field on an index (basis = ones and the
    index: coefficient 1 is the regression map).

    :param x: a `Forecast` (or anything with `.dims`, `.coords`, `.values`), a numpy array or a torch tensor.  Values on a HIP
        device are fitted there (dlwpcs_time_regression: fp64 normal equations in a fixed order) and the result stays there;
        numpy values are fitted on the host in float64 by the same rules, without a claim to the same bits.
    :param basis: host values, (T, K).  It is rounded to float32 ONCE, on both paths: the coefficients belong to the rounded
        basis, which is also what `regression_fitted` and `regression_residual` evaluate.
    :param axis: the axis to fit along, a position or a dim name; None: the 'time' dim of a labelled input, else axis 0
    :param missing: 'skip': fit the rows present.  'propagate': a grid point with a missing row is NaN.
    :param min_count: a grid point with fewer rows present is NaN (None: K).  So is one whose system is singular.
    :param return_count: also return the int32 number of rows present (no term dim)
    :return: float32 coefficients labelled like the input, a 'term' dim where the time axis stood
    """
    axis = _filter_axis(x, axis, 'time')
    b32 = _fit_basis32(basis, int(_raw(x).shape[axis]), 'time_regression')
    return _fit(x, b32, axis, missing, min_count, return_count, 'time_regression')


def _evaluate(coef, b32, term_axis, x, axis, name, rows_coord=None, row_dim='time'):
    """fitted values (x None) or residuals x - fitted, labelled"""
    c = _raw(coef)
    on_dev = _is_tensor(c) and c.is_cuda
    xv = None if x is None else _raw(x)
    if xv is not None and (_is_tensor(xv) and xv.is_cuda) != on_dev:
        raise ValueError('%s: the data and the coefficients must both be on the device or both on the host' % name)
    if on_dev:
        import torch
        from . import ops as dops
        with torch.cuda.device(c.device):
            cf = c if c.dtype == torch.float32 else c.to(torch.float32)
            src = None if xv is None else (xv if xv.dtype == torch.float32 else xv.to(torch.float32))
            out = dops.time_regression_apply(cf, b32, src=src, term_axis=term_axis, row_axis=axis)
    else:
        ch = np.moveaxis(np.asarray(_host(c), dtype=np.float64), term_axis, 0)
        with np.errstate(all='ignore'):
            f = np.tensordot(b32.astype(np.float64), ch, axes=(1, 0))
            bad = np.isnan(ch).any(axis=0)[None]
            if xv is None:
                y = np.moveaxis(np.where(bad, np.nan, f), 0, term_axis).astype(np.float32)
            else:
                xh = np.moveaxis(np.asarray(_host(xv), dtype=np.float64), axis, 0)
                y = np.moveaxis(np.where(bad, np.nan, xh - f), 0, axis).astype(np.float32)
    if x is not None:
        if not hasattr(x, 'dims'):
            return out if on_dev else y
        res = Forecast(out if on_dev else y, tuple(x.dims), {d: _coord(x, d) for d in x.dims if d in getattr(x, 'coords', {})}, name=name)
        if hasattr(x, 'lat'):
            res.lat = x.lat
        return res
    if not hasattr(coef, 'dims'):
        return out if on_dev else y
    dims = tuple(coef.dims)
    coords = {d: _coord(coef, d) for i, d in enumerate(dims) if i != term_axis and d in getattr(coef, 'coords', {})}
    if rows_coord is not None:
        coords[row_dim] = rows_coord
    res = Forecast(out if on_dev else y, dims[:term_axis] + (row_dim,) + dims[term_axis + 1:], coords, name=name)
    if hasattr(coef, 'lat'):
        res.lat = coef.lat
    return res


def regression_fitted(coef, basis, term_axis=None, times=None):
    """
    The fitted values sum_k basis[r, k] coef[k] of the coefficients of `time_regression` at the rows of `basis` (R, K; R need not
    be the length of the fit), in fp64 rounded to float32 once; NaN where the grid point's coefficients are.  A 'time' dim of R
    rows stands where the 'term' dim stood (its coordinate: `times`, when given).  Device coefficients are evaluated there.
    """
    term_axis = _filter_axis(coef, term_axis, 'term')
    b32 = _fit_basis32(basis, None, 'regression_fitted')
    if b32.shape[1] != int(_raw(coef).shape[term_axis]):
        raise ValueError('regression_fitted: %d coefficients, the basis has %d terms' % (_raw(coef).shape[term_axis], b32.shape[1]))
    return _evaluate(coef, b32, term_axis, None, term_axis, 'regression_fitted', None if times is None else np.asarray(times))


def regression_residual(x, coef, basis, axis=None, term_axis=None):
    """x minus the fitted values of `regression_fitted`, labelled like x: NaN where x or the grid point's coefficients are."""
    axis = _filter_axis(x, axis, 'time')
    term_axis = axis if term_axis is None and not hasattr(coef, 'dims') else _filter_axis(coef, term_axis, 'term')
    b32 = _fit_basis32(basis, int(_raw(x).shape[axis]), 'regression_residual')
    if b32.shape[1] != int(_raw(coef).shape[term_axis]):
        raise ValueError('regression_residual: %d coefficients, the basis has %d terms' % (_raw(coef).shape[term_axis], b32.shape[1]))
    return _evaluate(coef, b32, term_axis, x, axis, 'regression_residual')


def detrend(x, axis=None, order=1, missing='skip'):
    """
    x minus its least-squares polynomial of degree `order` (0 .. 3) along time, per grid point: powers of the row number centred
    and scaled to [-1, 1].  order 0 removes the mean of the rows present.  NaN where x is, and at a grid point with fewer than
    order + 1 rows present (with missing='propagate': with any row missing).
    """
    order = int(order)
    if not 0 <= order <= 3:
        raise ValueError('detrend: order %d outside 0 .. 3' % order)
    axis = _filter_axis(x, axis, 'time')
    T = int(_raw(x).shape[axis])
    t = _centred(np.arange(T))
    b32 = _fit_basis32(np.stack([t ** p for p in range(order + 1)], axis=1), T, 'detrend')
    coef = _fit(x, b32, axis, missing, None, False, 'detrend')
    return _evaluate(coef, b32, axis, x, axis, 'detrend')


class HarmonicClimatology(object):
    """
    A climatology as a mean, optionally a linear trend, and the first annual harmonics, fitted per grid point over a whole series
    (`harmonic_climatology`).  `.coefficients`: float32, a 'term' dim where the time dim stood, on the device when the data was.
    `.series(times)`: the climatology at any times, a 'time' dim in that place: what `daily_climo_time_series` returns, and
    accepted wherever that is.  `.anomalies(ds)`: ds minus the climatology at its own times.
    """

    def __init__(self, coefficients, n_harmonics, trend, span):
        self.coefficients = coefficients
        self.n_harmonics = int(n_harmonics)
        self.trend = bool(trend)
        self.span = span

    def basis(self, times):
        return harmonic_basis(times, self.n_harmonics, self.trend, trend_span=self.span)

    def series(self, times, f_hour=None):
        """the climatology at `times`; with `f_hour` at times + f_hour, behind a leading 'f_hour' dim, as daily_climo_time_series"""
        t = np.asarray(getattr(times, 'values', times))
        axis = _filter_axis(self.coefficients, None, 'term')
        if f_hour is None:
            b32 = _fit_basis32(self.basis(t), None, 'harmonic_climatology')
            return _evaluate(self.coefficients, b32, axis, None, axis, 'climatology', t)
        when = t.astype('datetime64[s]')[None, :] + _lead_hours(f_hour).astype('timedelta64[s]')[:, None]
        b32 = _fit_basis32(self.basis(when.reshape(-1)), None, 'harmonic_climatology')
        flat = _evaluate(self.coefficients, b32, axis, None, axis, 'climatology', when.reshape(-1))
        v = _raw(flat)
        v = v.reshape(tuple(v.shape[:axis]) + when.shape + tuple(v.shape[axis + 1:]))
        v = v.movedim(axis, 0) if _is_tensor(v) else np.moveaxis(v, axis, 0)
        if not hasattr(flat, 'dims'):
            return v
        coords = {d: c for d, c in flat.coords.items() if d != 'time'}
        coords['time'] = t
        coords['f_hour'] = np.asarray(getattr(f_hour, 'values', f_hour))
        out = Forecast(v, ('f_hour',) + tuple(flat.dims), coords, name='climatology')
        if hasattr(flat, 'lat'):
            out.lat = flat.lat
        return out

    def anomalies(self, ds):
        axis = _filter_axis(ds, None, 'time')
        if not (hasattr(ds, 'coords') and 'time' in ds.coords):
            raise ValueError("harmonic_climatology: the data has no 'time' coordinate")
        b32 = _fit_basis32(self.basis(_coord(ds, 'time')), int(_raw(ds).shape[axis]), 'harmonic_climatology')
        return _evaluate(self.coefficients, b32, _filter_axis(self.coefficients, None, 'term'), ds, axis, 'anomaly')


def harmonic_climatology(ds, n_harmonics=4, trend=False, min_count=None):
    """
    The harmonic climatology of a labelled series with a datetime64 'time' coordinate: a mean, with `trend` a linear trend, and
    `n_harmonics` harmonics of the tropical year, fitted per grid point to the rows that are not NaN (`time_regression`).  Where
    `daily_climatology` averages the thirty-odd values a day of the year has, this fits 1 + 2 n_harmonics numbers to all of them.
    Returns a `HarmonicClimatology`.
    """
    if not (hasattr(ds, 'dims') and 'time' in tuple(ds.dims) and 'time' in getattr(ds, 'coords', {})):
        raise ValueError("harmonic_climatology: the data needs a 'time' dimension with a coordinate")
    t = _coord(ds, 'time')
    if t.dtype.kind != 'M':
        raise ValueError("harmonic_climatology: the 'time' coordinate must be datetime64")
    span = (t.min(), t.max()) if t.size else None
    basis = harmonic_basis(t, n_harmonics, trend, trend_span=span)
    axis = tuple(ds.dims).index('time')
    coef = _fit(ds, _fit_basis32(basis, int(_raw(ds).shape[axis]), 'harmonic_climatology'), axis, 'skip', min_count, False,
                'harmonic_climatology')
    return HarmonicClimatology(coef, n_harmonics, trend, span)


# --------------------------------------------------------------------------------------------------------------------- #
# Spectra along time: Welch's power spectrum, cross-spectra and coherence, wavenumber-frequency diagrams
# --------------------------------------------------------------------------------------------------------------------- #
#
# A series is cut into segments of n_segment rows, `hop` rows apart; a segment is (optionally) freed of its mean, multiplied by
# a window w and transformed: X_f = sum_t w_t x_t exp(-2 pi i f t / M).  P_f = c_f |X_f|^2 / (M S_w), S_w = sum w_t^2, c_f = 1 at
# f = 0 and at the Nyquist frequency of an even M, else 2, so that sum_f P_f is the window-weighted mean square of the segment;
# the result is the mean over the segments whose values are all finite.  numpy values are transformed on the host in float64
# with np.fft.rfft, device tensors by dlwpcs_time_spectrum (fp32 on the matrix cores, fp64 segment sums in a fixed order) and
# stay there as float32; neither path falls back to the other.  Both use the window rounded to float32.  The new dim is
# 'frequency', in cycles per row.

TimeCrossSpectrum = namedtuple('TimeCrossSpectrum', ['power_a', 'power_b', 'co', 'quad'])
WavenumberFrequencySpectrum = namedtuple('WavenumberFrequencySpectrum', ['eastward', 'westward'])


def spectral_window(window, n):
    """
    n float64 window weights: 'boxcar' (ones), 'hann' (periodic: 0.5 - 0.5 cos(2 pi t / n), the form that overlaps to a constant
    at hop n / 2), or an array of n weights, returned as it is.  Host only.
    """
    n = int(n)
    if n < 1:
        raise ValueError('spectral_window: %d weights' % n)
    if isinstance(window, str):
        if window == 'boxcar':
            return np.ones(n, dtype=np.float64)
        if window == 'hann':
            return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / n)
        raise ValueError("spectral_window: 'window' must be 'boxcar', 'hann' or an array of weights, got %r" % (window,))
    w = np.asarray(_host(window), dtype=np.float64).reshape(-1)
    if w.size != n:
        raise ValueError('spectral_window: %d weights for segments of %d rows' % (w.size, n))
    return w


def _welch_args(x, n_segment, axis, hop, window, detrend, n_freq, min_count, name, whole=False):
    """(axis, M, hop, float64 window rounded to float32, its sum of squares, detrend flag, K, min_count)"""
    ax = _filter_axis(x, axis, 'time')
    T = int(_raw(x).shape[ax])
    if n_segment is None and not whole:
        raise ValueError('%s: n_segment is needed' % name)
    M = T if n_segment is None else int(n_segment)
    if M < 2:
        raise ValueError('%s: segments of %d rows (at least 2)' % (name, M))
    hop = max(1, M // 2) if hop is None else int(hop)
    if hop < 1:
        raise ValueError('%s: hop must be at least 1, got %d' % (name, hop))
    if detrend not in (None, 'constant'):
        raise ValueError("%s: 'detrend' must be None or 'constant' (remove a linear trend from the whole series with detrend())" % name)
    K = M // 2 + 1 if n_freq is None else int(n_freq)
    if not 1 <= K <= M // 2 + 1:
        raise ValueError('%s: n_freq = %s outside 1 .. n_segment // 2 + 1 = %d' % (name, n_freq, M // 2 + 1))
    if int(min_count) < 1:
        raise ValueError('%s: min_count must be at least 1, got %d' % (name, min_count))
    with np.errstate(over='ignore'):
        w = spectral_window(window, M).astype(np.float32).astype(np.float64)
    sw = float((w ** 2).sum())
    if not np.all(np.isfinite(w)) or not sw > 0.:
        raise ValueError('%s: the window must be finite in float32 with a positive sum of squares' % name)
    return ax, M, hop, w, sw, detrend == 'constant', K, int(min_count)


def _segment_count(T, M, hop):
    return (T - M) // hop + 1 if T >= M else 0


def _fourier_host(v, M, hop, w, detrend, K):
    """(coefficients (n_seg, K, ...) complex128, counted (n_seg, ...) bool) of v (T, ...) float64"""
    n_seg = _segment_count(v.shape[0], M, hop)
    X = np.full((n_seg, K) + v.shape[1:], complex(np.nan, np.nan), dtype=np.complex128)
    ok = np.zeros((n_seg,) + v.shape[1:], dtype=bool)
    ws = w.reshape((M,) + (1,) * (v.ndim - 1))
    for s in range(n_seg):
        seg = v[s * hop:s * hop + M]
        ok[s] = np.isfinite(seg).all(axis=0)
        z = np.where(ok[s], seg, 0.0)
        if detrend:
            z = z - z.mean(axis=0)
        X[s] = np.where(ok[s], np.fft.rfft(z * ws, axis=0)[:K], complex(np.nan, np.nan))
    return X, ok


def _spectral_scale(M, K, sw):
    c = np.full(K, 2.0)
    c[0] = 1.0
    if M % 2 == 0 and K == M // 2 + 1:
        c[-1] = 1.0
    return c / (M * sw)


def _welch_host(a, b, ax, M, hop, w, sw, detrend, K, min_count):
    """numpy twin of dlwpcs_time_spectrum: (quantities (nq, ...) float64 with K frequencies at `ax`, counts int32 without it)"""
    A, ok = _fourier_host(np.moveaxis(np.asarray(a, dtype=np.float64), ax, 0), M, hop, w, detrend, K)
    if b is not None:
        B, okb = _fourier_host(np.moveaxis(np.asarray(b, dtype=np.float64), ax, 0), M, hop, w, detrend, K)
        ok = ok & okb
    q = [A.real ** 2 + A.imag ** 2]
    if b is not None:
        cross = A * np.conj(B)
        q += [B.real ** 2 + B.imag ** 2, cross.real, cross.imag]
    n = ok.sum(axis=0).astype(np.int32)
    scale = _spectral_scale(M, K, sw).reshape((K,) + (1,) * (A.ndim - 2))
    with np.errstate(invalid='ignore', divide='ignore'):
        out = np.stack([np.where(n >= min_count, np.where(ok[:, None], x, 0.0).sum(axis=0) * scale / np.maximum(n, 1), np.nan)
                        for x in q])
    return np.moveaxis(out, 1, ax + 1), n


def _device_f32(x):
    import torch
    v = _raw(x)
    return v if v.dtype == torch.float32 else v.to(torch.float32)


def _welch(a, b, n_segment, axis, hop, window, detrend, n_freq, min_count, name):
    """(quantities (nq, ...), counts, axis, M): numpy float64 for host values, float32 device tensors for device values"""
    if b is not None:
        _check_labels(a, b)
        if tuple(_raw(a).shape) != tuple(_raw(b).shape):
            raise ValueError('%s: the two series %s and %s must have one shape' % (name, tuple(_raw(a).shape), tuple(_raw(b).shape)))
    ax, M, hop, w, sw, dt, K, mc = _welch_args(a, n_segment, axis, hop, window, detrend, n_freq, min_count, name)
    if _on_device(a, b):
        import torch
        from . import ops as dops
        dev = next(_raw(x).device for x in (a, b) if x is not None and _is_tensor(_raw(x)) and _raw(x).is_cuda)
        with torch.cuda.device(dev):
            at = _dev_operand(a, dev)
            bt = _dev_operand(b, dev) if b is not None else None
            out, cnt = dops.time_spectrum(at, bt, n_segment=M, hop=hop, window=w, row_axis=ax, detrend=dt, n_freq=K, min_count=mc,
                                          counts=True)
        return (out if b is not None else out[None]), cnt, ax, M
    out, cnt = _welch_host(_host(a), None if b is None else _host(b), ax, M, hop, w, sw, dt, K, mc)
    return out, cnt, ax, M


def _freq_label(x, axis, values, M, name, renamed=None, lead=()):
    """`values` labelled like x with 'frequency' (cycles per row) where `axis` stood; renamed: {axis: (dim, coordinate)} for
    further axes that changed their meaning; lead: names of leading dims of `values` that x does not have"""
    if not hasattr(x, 'dims'):
        return values
    renamed = dict(renamed or {})
    renamed[axis] = ('frequency', np.arange(values.shape[len(lead) + axis]) / float(M))
    dims, coords = [], {}
    for i, d in enumerate(tuple(x.dims)):
        if i in renamed:
            d, c = renamed[i]
            if c is not None:
                coords[d] = c
        elif d in getattr(x, 'coords', {}):
            coords[d] = _coord(x, d)
        dims.append(d)
    out = Forecast(values, tuple(lead) + tuple(dims), coords, name=name)
    if hasattr(x, 'lat'):
        out.lat = x.lat
    return out


def _drop_label(x, axis, values, name):
    """`values` (x's shape without `axis`) labelled like x without that dim"""
    if not hasattr(x, 'dims'):
        return values
    dims = tuple(d for i, d in enumerate(x.dims) if i != axis)
    coords = {d: _coord(x, d) for d in dims if d in getattr(x, 'coords', {})}
    return Forecast(values, dims, coords, name=name)


def time_spectrum(x, n_segment, axis=None, hop=None, window='hann', detrend='constant', n_freq=None, min_count=1, return_count=False):
    """
    Welch's power spectrum of a series along time: the mean over segments of `n_segment` rows of P_f = c_f |X_f|^2 / (M S_w),
    whose sum over all frequencies is the window-weighted mean square of a segment (its variance with detrend='constant').

    :param x: a `Forecast` (or anything with `.dims`, `.coords`, `.values`), a numpy array or a torch tensor.  Values on a HIP
        device are transformed there (dlwpcs_time_spectrum) and the float32 result stays there; numpy values are transformed on
        the host in float64
    :param n_segment: rows per segment, M (on the device at most 1728)
    :param axis: the axis to transform, a position or a dim name; None: the 'time' dim of a labelled input, else axis 0
    :param hop: rows between the starts of neighbouring segments; None: n_segment // 2, the half overlap that suits 'hann'
    :param window: 'hann' (periodic), 'boxcar' or an array of n_segment weights (`spectral_window`); used rounded to float32
    :param detrend: 'constant': every segment loses its own mean; None: nothing.  A linear trend is removed from the whole series
        with the existing `detrend()` first
    :param n_freq: return the first n_freq frequencies only (1 .. n_segment // 2 + 1)
    :param min_count: a segment counts where all its values are finite; NaN where fewer than min_count segments count (also where
        the series is shorter than one segment)
    :param return_count: also return the int32 number of segments that counted (the input's shape without the time axis)
    :return: labelled like the input with the dim 'frequency' (cycles per row) where the time axis stood
    """
    out, cnt, ax, M = _welch(x, None, n_segment, axis, hop, window, detrend, n_freq, min_count, 'time_spectrum')
    res = _freq_label(x, ax, out[0], M, 'time_spectrum')
    return (res, _drop_label(x, ax, cnt, 'time_spectrum_count')) if return_count else res


def time_cross_spectrum(a, b, n_segment, axis=None, hop=None, window='hann', detrend='constant', n_freq=None, min_count=1,
                        return_count=False):
    """
    The power spectra of two series of one shape and their cross-spectrum along time, averaged over the segments that are finite
    in both: TimeCrossSpectrum(power_a, power_b, co, quad) with co + i quad = c_f A_f conj(B_f) / (M S_w).  Arguments as for
    `time_spectrum`.
    """
    out, cnt, ax, M = _welch(a, b, n_segment, axis, hop, window, detrend, n_freq, min_count, 'time_cross_spectrum')
    res = TimeCrossSpectrum(*[_freq_label(a, ax, out[i], M, n) for i, n in enumerate(TimeCrossSpectrum._fields)])
    return (res, _drop_label(a, ax, cnt, 'time_cross_spectrum_count')) if return_count else res


def time_coherence(a, b, n_segment, axis=None, hop=None, window='hann', detrend='constant', n_freq=None, min_count=1,
                   return_count=False):
    """
    Squared coherence (co^2 + quad^2) / (power_a power_b) per frequency, formed from the segment-AVERAGED spectra of
    `time_cross_spectrum` (per segment it would be identically 1): 1 where the forecast holds the verification's phase over the
    segments, near 1 / segments where the two are unrelated.  NaN where either power is 0.  Arguments as for `time_spectrum`.
    """
    out, cnt, ax, M = _welch(a, b, n_segment, axis, hop, window, detrend, n_freq, min_count, 'time_coherence')
    if _is_tensor(out):
        den = out[0] * out[1]
        coh = (out[2] ** 2 + out[3] ** 2) / den
        coh = coh.masked_fill(den == 0, float('nan'))
    else:
        with np.errstate(invalid='ignore', divide='ignore'):
            coh = np.where(out[0] * out[1] == 0, np.nan, (out[2] ** 2 + out[3] ** 2) / (out[0] * out[1]))
    res = _freq_label(a, ax, coh, M, 'time_coherence')
    return (res, _drop_label(a, ax, cnt, 'time_coherence_count')) if return_count else res


def time_fourier(x, axis=None, n_segment=None, hop=None, window='boxcar', detrend=None, n_freq=None):
    """
    The complex coefficients X_f = sum_t w_t x_t exp(-2 pi i f t / M) per segment, unscaled: what `time_spectrum` averages the
    squares of, and what a transform along one axis feeds to a second transform along another.  n_segment=None: one segment over
    the whole axis (on the device at most 1728 rows) and no segment axis; else a leading 'segment' axis.  A segment that holds a
    value that is not finite is NaN.  complex128 for host values; complex64 on the device for device values.  Other arguments as
    for `time_spectrum`.
    """
    ax, M, hop, w, sw, dt, K, _ = _welch_args(x, n_segment, axis, hop, window, detrend, n_freq, 1, 'time_fourier', whole=True)
    v = _raw(x)
    if _is_tensor(v) and v.is_cuda:
        import torch
        from . import ops as dops
        with torch.cuda.device(v.device):
            z = dops.time_fourier(_device_f32(x), n_segment=M, hop=hop, window=w, row_axis=ax, detrend=dt, n_freq=K)
            out = torch.view_as_complex(z.movedim(ax + 2, -1).contiguous())
    else:
        X, _ = _fourier_host(np.moveaxis(np.asarray(_host(v), dtype=np.float64), ax, 0), M, hop, w, dt, K)
        out = np.moveaxis(X, 1, ax + 1)
    if n_segment is None:
        return _freq_label(x, ax, out[0], M, 'time_fourier')
    return _freq_label(x, ax, out, M, 'time_fourier', lead=('segment',))


def _mirror(x, lat_axis, component, name):
    """(x + flip) / 2 or (x - flip) / 2 along lat_axis: the part symmetric or antisymmetric about the equator"""
    if component not in ('symmetric', 'antisymmetric'):
        raise ValueError("%s: 'component' must be None, 'symmetric' or 'antisymmetric'" % name)
    if lat_axis is None:
        raise ValueError('%s: a component needs a latitude axis' % name)
    if hasattr(x, 'coords') and hasattr(x, 'dims') and x.dims[lat_axis] in x.coords:
        lat = np.asarray(_coord(x, x.dims[lat_axis]), dtype=np.float64)
        if not np.allclose(lat, -lat[::-1], rtol=0., atol=1e-6 * max(1., float(np.abs(lat).max()))):
            raise ValueError('%s: the latitudes do not mirror about the equator' % name)
    v = _raw(x)
    f = v.flip(lat_axis) if _is_tensor(v) else np.flip(v, lat_axis)
    return (v + f) * 0.5 if component == 'symmetric' else (v - f) * 0.5


def wavenumber_frequency_spectrum(x, n_segment, axis=None, lon_axis=-1, lat_axis=None, component=None, hop=None, window='hann',
                                  detrend='constant', n_wave=None, n_freq=None, min_count=1, return_count=False):
    """
    The wavenumber-frequency power of a series of fields (Wheeler and Kiladis 1999): per zonal wavenumber k and frequency f the
    variance that travels eastward and westward, WavenumberFrequencySpectrum(eastward, westward), each with 'frequency' where the
    time axis stood and 'wavenumber' where longitude stood; every other axis (latitude) is kept: reducing it is the caller's.

    Stage 1 is the zonal transform X_k(t) of every row (`time_fourier` along longitude: one boxcar segment); stage 2 the pair form
    of `time_spectrum` along time on its real and imaginary planes a, b (window, detrend, hop and the missing-value rule as there),
    and with c_k the factor of `zonal_spectrum`
        westward = (P_aa + P_bb + 2 Q) / 2 * c_k / L^2,      eastward = (P_aa + P_bb - 2 Q) / 2 * c_k / L^2,
    Q the quadrature spectrum.  A wave cos(k lon - 2 pi f t / M) lands in eastward[f, k] alone; eastward.sum() + westward.sum()
    over all k and f is the window-weighted mean square of the segments; f = 0 and the Nyquist frequency hold half in each.

    :param lon_axis: the longitude axis (the dim 'lon' of a labelled input); on the device at most 1728 longitudes
    :param lat_axis: the latitude axis, needed for `component` only (None: the dim 'lat' of a labelled input, if any)
    :param component: None, or 'symmetric' / 'antisymmetric': (x +- x mirrored about the equator) / 2 is analysed; the latitudes
        must mirror
    :param n_wave: the first n_wave zonal wavenumbers only (1 .. L // 2 + 1)
    Other arguments as for `time_spectrum`.  The same pair form serves any complex series c(t): for `spherical_analysis`
    coefficients `coef` (..., 2) interleaved, time_cross_spectrum(coef[..., 0], coef[..., 1], n_segment) reads the two planes in
    place (inner stride 2) and (power_a + power_b -+ 2 quad) / 2 are the powers of the two directions of rotation.
    """
    name = 'wavenumber_frequency_spectrum'
    ax = _filter_axis(x, axis, 'time')
    lon = _lon_axis(x, lon_axis)
    nd = len(_raw(x).shape)
    if lon == ax:
        raise ValueError('%s: time and longitude are one axis' % name)
    if lat_axis is None and hasattr(x, 'dims') and 'lat' in tuple(x.dims):
        lat_axis = tuple(x.dims).index('lat')
    if lat_axis is not None:
        lat_axis = _axes(lat_axis, nd)[0]
        if lat_axis in (ax, lon):
            raise ValueError('%s: the latitude axis is the time or the longitude axis' % name)
    L = int(_raw(x).shape[lon])
    if L < 2:
        raise ValueError('%s: %d longitudes (at least 2)' % (name, L))
    Kw = L // 2 + 1 if n_wave is None else int(n_wave)
    if not 1 <= Kw <= L // 2 + 1:
        raise ValueError('%s: n_wave = %s outside 1 .. L // 2 + 1 = %d' % (name, n_wave, L // 2 + 1))
    _, M, hop, w, sw, dt, K, mc = _welch_args(x, n_segment, ax, hop, window, detrend, n_freq, min_count, name)
    v = _raw(x) if component is None else _mirror(x, lat_axis, component, name)
    ck = np.full(Kw, 2.0)
    ck[0] = 1.0
    if L % 2 == 0 and Kw == L // 2 + 1:
        ck[-1] = 1.0
    shape = [1] * nd
    shape[lon] = Kw
    ck = (ck / (2.0 * float(L) ** 2)).reshape(shape)
    if _is_tensor(v) and v.is_cuda:
        import torch
        from . import ops as dops
        with torch.cuda.device(v.device):
            src = v if v.dtype == torch.float32 else v.to(torch.float32)
            z = dops.time_fourier(src, row_axis=lon, n_freq=Kw)[0].movedim(lon + 1, -1)     # (..., wavenumber, ..., 2)
            p, cnt = dops.time_spectrum(z[..., 0], z[..., 1], n_segment=M, hop=hop, window=w, row_axis=ax, detrend=dt, n_freq=K,
                                        min_count=mc, counts=True)
            ckt = torch.from_numpy(ck.astype(np.float32)).to(v.device)
            both = (p[0] + p[1]) * ckt
            twoq = (2.0 * p[3]) * ckt
            east, west = both - twoq, both + twoq
    else:
        h = np.asarray(_host(v), dtype=np.float64)
        rows_ok = np.isfinite(h).all(axis=lon, keepdims=True)
        z = np.fft.rfft(np.where(rows_ok, h, 0.0), axis=lon)
        z = np.where(rows_ok, np.take(z, np.arange(Kw), axis=lon), complex(np.nan, np.nan))
        p, cnt = _welch_host(z.real, z.imag, ax, M, hop, w, sw, dt, K, mc)
        east, west = (p[0] + p[1] - 2.0 * p[3]) * ck, (p[0] + p[1] + 2.0 * p[3]) * ck
    ren = {lon: ('wavenumber', np.arange(Kw))}
    res = WavenumberFrequencySpectrum(_freq_label(x, ax, east, M, 'eastward', ren), _freq_label(x, ax, west, M, 'westward', ren))
    if not return_count:
        return res
    if hasattr(x, 'dims'):
        dims = tuple('wavenumber' if i == lon else d for i, d in enumerate(x.dims) if i != ax)
        coords = {d: _coord(x, d) for d in dims if d in getattr(x, 'coords', {})}
        coords['wavenumber'] = np.arange(Kw)
        cnt = Forecast(cnt, dims, coords, name=name + '_count')
    return res, cnt
