"""
What a labelled array is, in one place: the `Forecast` record (values, dimension names, one coordinate array per dimension --
the subset of xarray.DataArray the engine reads; xarray is not part of this stack), and the three things every analysis family
does with one -- get at the values behind it (`raw`, `host`, `on_device`, `device_f32`, `device_scope`), find an axis from a
position or a dim name (`axis_of`, `axes`), and label a result like its input (`label`).

A leaf: numpy only, nothing of DLWP, and torch only where a caller has already brought it in.
"""
import sys

import numpy as np


class Forecast(object):
    """values + named dims + coordinate arrays (the subset of xarray.DataArray the verification code reads)."""

    def __init__(self, values, dims, coords, name='forecast'):
        self.values = values
        self.dims = tuple(dims)
        self.coords = dict(coords)
        self.name = name

    @property
    def shape(self):
        return self.values.shape

    def __array__(self, dtype=None, copy=None):
        v = self.values
        if hasattr(v, 'detach'):                                  # device-resident values (predict(keep_on_device=True))
            v = v.detach().cpu().numpy()
        return np.asarray(v, dtype=dtype)

    def isel(self, **indexers):
        idx = [slice(None)] * self.values.ndim
        coords = dict(self.coords)
        for k, v in indexers.items():
            ax = self.dims.index(k)
            idx[ax] = v
            coords[k] = np.asarray(self.coords[k])[v]
        vals = self.values[tuple(idx)]
        dims = tuple(d for d, i in zip(self.dims, idx) if not isinstance(i, (int, np.integer)))
        return Forecast(vals, dims, {d: coords[d] for d in dims if d in coords}, self.name)


# ---- the values behind an input ------------------------------------------------------------------------------------- #

def is_tensor(x):
    torch = sys.modules.get('torch')
    return torch is not None and isinstance(x, torch.Tensor)


def raw(x):
    """the array behind a wrapped input (a Forecast / DataArray: `.values`), else x itself"""
    if isinstance(x, np.ndarray) or is_tensor(x):
        return x
    return getattr(x, 'values', x)


def on_device(*xs):
    return any(is_tensor(raw(x)) and raw(x).is_cuda for x in xs if x is not None)


def host(x):
    r = raw(x)
    if hasattr(r, 'detach'):
        r = r.detach().cpu().numpy()
    return np.asarray(r)


def device_f32(x):
    """the fp32 device tensor behind x: the tensor itself when it is one, else converted under its device's context"""
    import torch
    v = raw(x)
    if v.dtype == torch.float32:
        return v
    with torch.cuda.device(v.device):
        return v.to(torch.float32)


class device_scope(object):
    """`with device_scope(a, b) as dev:` -- the context of the device the first device-resident input lies on"""

    def __init__(self, *xs):
        import torch
        self.device = next(raw(x).device for x in xs if x is not None and on_device(x))
        self._context = torch.cuda.device(self.device)

    def __enter__(self):
        self._context.__enter__()
        return self.device

    def __exit__(self, *exc):
        return self._context.__exit__(*exc)


# ---- axes ------------------------------------------------------------------------------------------------------------- #

def axis_of(x, dim, position=0, out_of_range='axis %d is out of range of %d dims', explicit=None, missing=None):
    """
    The position of one axis of x.

    :param dim: the dim name looked for on a labelled input; where x has it, that is the axis
    :param position: the axis of an unlabelled input, and of a labelled one without `dim`; range-checked
    :param out_of_range: the message of that check, formatted with (position, number of axes)
    :param explicit: an `axis=` argument of the caller's that outranks `dim` (the families along time): None leaves the rules
        above, a dim name must be one of x's, a position is range-checked
    :param missing: where given, a labelled input must have `dim`; the message, formatted with the tuple of x's dims
    """
    dims = tuple(getattr(x, 'dims', ()))
    if isinstance(explicit, str):
        if explicit not in dims:
            raise ValueError("the data has no '%s' dimension (dims: %s)" % (explicit, ', '.join(dims)))
        return dims.index(explicit)
    if explicit is None:
        if dim in dims:
            return dims.index(dim)
        if missing is not None and hasattr(x, 'dims'):
            raise ValueError(missing % (dims,))
    nd = len(raw(x).shape)
    a = int(position if explicit is None else explicit)
    if a < -nd or a >= nd:
        raise ValueError(out_of_range % (a, nd))
    return a % nd


def axes(axis, nd, src=None):
    """None, or the tuple of the positions `axis` names among nd axes: an int or a sequence of them, negative ones counted from
    the end, none twice; with a labelled `src`, dim names too"""
    if axis is None:
        return None
    single = (int, np.integer) if src is None else (int, np.integer, str)
    out = []
    for a in ((axis,) if isinstance(axis, single) else tuple(axis)):
        a = tuple(src.dims).index(a) if src is not None and isinstance(a, str) else int(a)
        if a < -nd or a >= nd:
            raise np.exceptions.AxisError(a, nd) if hasattr(np, 'exceptions') else ValueError('axis %d out of range' % a)
        out.append(a % nd)
    if len(set(out)) != len(out):
        raise ValueError('duplicate value in axis')
    return tuple(out)


# ---- labels ----------------------------------------------------------------------------------------------------------- #

def coord(src, d):
    """the coordinate of dim d as a numpy array"""
    return np.asarray(getattr(src.coords[d], 'values', src.coords[d]))


def labels(src, drop=(), replace=None, select=None, lead=(), tail=()):
    """(dims, coords) of a result derived from the labelled `src`; the arguments are those of `label`"""
    replace, select, have = replace or {}, select or {}, getattr(src, 'coords', {})
    dims, coords = [], {}
    for i, d in enumerate(tuple(src.dims)):
        if i in drop:
            continue
        if i in replace:
            d, c = replace[i]
        else:
            c = coord(src, d) if d in have else None
            if c is not None and i in select:
                c = c[select[i]]
        dims.append(d)
        if c is not None:
            coords[d] = c
    for d, c in tuple(lead) + tuple(tail):
        if c is not None:
            coords[d] = np.asarray(c)
    return tuple(d for d, _ in lead) + tuple(dims) + tuple(d for d, _ in tail), coords


def label(src, values, name, drop=(), replace=None, select=None, lead=(), tail=(), lat=False):
    """
    `values` labelled like the input `src` it was computed from: a `Forecast` named `name` over the dims of `src`, each with the
    coordinate `src` has for it (a dim without one gets none).  An unlabelled `src` returns `values` as they are.

    :param drop: positions among the dims of `src` that the result no longer has
    :param replace: {position: (dim, coordinate or None)}: the dim that stands there now
    :param select: {position: rows}: the coordinate there taken at these rows
    :param lead, tail: sequences of (dim, coordinate or None): new dims in front of and behind those of `src`
    :param lat: carry `src.lat` (the latitudes `weighted=True` reads) over to the result

    Who carries `.lat` is inherited from the families as they were written, not designed: the climatology tables
    (`daily_climatology`, `climatology_quantiles`), the categorical scores (`ensemble_probability`, `brier_score`,
    `ranked_probability_score`, `reliability_counts`), the time filters, the fits and what is evaluated from them, and the time
    spectra do; the series and anomalies laid out from a climatology table, the zonal and spherical families, the per-element
    ensemble statistics and the segment counts of the time spectra do not.
    """
    if not hasattr(src, 'dims'):
        return values
    out = Forecast(values, *labels(src, drop, replace, select, lead, tail), name=name)
    if lat and hasattr(src, 'lat'):
        out.lat = src.lat
    return out
