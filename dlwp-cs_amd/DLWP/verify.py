"""
Scoring forecasts (reference DLWP/verify.py:18-164: `forecast_error`, `persistence_error`, `climo_error`) and labelling a
cubed-sphere forecast array (behaviour of reference DLWP/verify.py:291-325, pinned by tests/golden/g11_verify.npz:
dimension names and order, coordinate values, the split of the channel axis into variable x level).

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
    :param climatology: climatology for 'acc' / 'cos'
    :return: float64 ndarray with forecast hour as the first dimension
    """
    assert method in _METHODS, _METHOD_MSG
    if method in ['acc', 'cos'] and climatology is None:
        warnings.warn("'acc' and 'cos' error methods expect to get a climatology; using 0 instead, which may yield "
                      "unexpected results.")
        climatology = 0.
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
