"""
Per-variable data scaling of the MI355X engine (reference DLWP/model/preprocessing.py): the statistics that
`Preprocessor.data_to_series(scale_variables=True)` stores per variable/level (:645-682, `mean_by_batch` / `std_by_batch` at
:844-882), the transform `(x - mean) / std` it applies to the predictors (:660), and the inverse `x * std + mean` that
Tutorial 4 (cell 19) applies to every forecast before anything physical is reported.

A numpy array is served on the host; a HIP tensor (the resident training array, a `predict(keep_on_device=True)` forecast)
is served where it lies by one streaming pass per step: `ops.channel_moments` (fp64 sums, fixed order) for the statistics,
`ops.channel_affine` (two rounded fp32 operations per element, the layout may change in the same pass) for the transforms.
Differences from the reference: the statistics file is not read (the tables are numpy arrays; netCDF-4 storage is not part
of this stack), the sums are fp64 where the reference adds float32 batch sums, and `Preprocessor`, `get_constants` and
`prepare_data_array` (xarray / netCDF4 file handling) are not built.
"""
import numpy as np

from ..labelled import Forecast, host as _host, is_tensor as _is_tensor, on_device, raw as _raw


def _device_values(x):
    return _raw(x) if on_device(x) else None


def _as_rows(v):
    """a device tensor as (rows, 1, rest...): one channel, the first dim kept as the row dim"""
    if v.dim() < 2:
        return v.reshape(1, 1, -1)
    return v.unsqueeze(1)


def mean_by_batch(da, batch_size, axis=0):
    """
    Loop over batches indexed in axis to take the grand mean of the array in a memory-efficient way (reference
    DLWP/model/preprocessing.py:844-860).  Sums are float64 (the reference adds float32 batch sums).

    :param da: numpy array, torch tensor or anything with `.values`; a HIP tensor (float32) is reduced on the device in one pass,
        where batch_size is ignored
    :param batch_size: int: number of samples to load and mean at a time
    :param axis: int: axis along which to index batches
    :return: float: the mean of the array
    """
    v = _device_values(da)
    if v is not None:
        from .. import ops
        m = ops.channel_moments(_as_rows(v), axis=1, as_numpy=True)[0]
        return float(m[1] / v.numel())
    x = _host(da)
    size = x.shape[axis]
    total = 0.0
    for b in range(0, size, batch_size):
        idx = [slice(None)] * x.ndim
        idx[axis] = slice(b, min(b + batch_size, size))
        total += float(np.sum(x[tuple(idx)], dtype=np.float64))
    return total / x.size


def std_by_batch(da, batch_size, axis=0, mean=None):
    """
    Loop over batches indexed in axis to take the standard deviation of the array in a memory-efficient way.  If mean is
    provided, assumes the mean of the data is already known to be this value (reference DLWP/model/preprocessing.py:863-882:
    sqrt(sum((x - mean)^2) / size), ddof 0).  Without it a first pass computes it, as the reference does.

    :param da: numpy array, torch tensor or anything with `.values`; a HIP tensor (float32) takes one device pass per sum, where
        batch_size is ignored
    :param batch_size: int: number of samples to load and mean at a time
    :param axis: int: axis along which to index batches
    :param mean: float: the (known) mean of the array
    :return: float: the standard deviation of the array
    """
    if mean is None:
        mean = mean_by_batch(da, batch_size, axis)
    v = _device_values(da)
    if v is not None:
        from .. import ops
        m = ops.channel_moments(_as_rows(v), axis=1, center=[float(mean)], as_numpy=True)[0]
        return float(np.sqrt(m[2] / v.numel()))
    x = _host(da)
    size = x.shape[axis]
    total = 0.0
    for b in range(0, size, batch_size):
        idx = [slice(None)] * x.ndim
        idx[axis] = slice(b, min(b + batch_size, size))
        d = x[tuple(idx)].astype(np.float64) - float(mean)
        total += float(np.sum(d * d))
    return float(np.sqrt(total / x.size))


def _moments_host(x, axis, rows, center, skipna):
    """(C, 3) float64 {n, sum (x - center), sum (x - center)^2} per entry of `axis`, one variable at a time"""
    if rows is not None:
        x = x[np.asarray(rows, dtype=np.int64).reshape(-1)]
    C = x.shape[axis]
    out = np.zeros((C, 3), dtype=np.float64)
    for c in range(C):
        d = np.take(x, c, axis=axis).astype(np.float64)
        if center is not None:
            d = d - center[c]
        if skipna:
            d = d[~np.isnan(d)]
        out[c] = (d.size, d.sum(), (d * d).sum())
    return out


def _moments(array, axis, rows, center, skipna):
    v = _device_values(array)
    if v is not None:
        from .. import ops
        return ops.channel_moments(v, axis=axis, rows=rows, center=center, skipna=skipna, as_numpy=True)
    x = _host(array)
    axis = axis % x.ndim
    if rows is not None and axis == 0:
        raise ValueError('variable_statistics: a row list selects entries of axis 0, which is the variable axis here')
    return _moments_host(x, axis, rows, center, skipna)


def variable_statistics(array, axis=1, rows=None, skipna=False, center=None):
    """
    Mean and standard deviation (ddof 0) of every variable along `axis`, over all other axes: the numbers
    `Preprocessor.data_to_series(scale_variables=True)` stores per `varlev` (reference DLWP/model/preprocessing.py:648-651).

    :param array: numpy array, HIP tensor (float32; one launch pair per pass for all variables) or anything with `.values`
    :param axis: int: the variable axis
    :param rows: optional ints: the entries of the FIRST axis that take part (statistics belong to the training period);
        duplicates count as given
    :param skipna: bool: leave NaN elements out (else one NaN makes its variable's statistics NaN, as numpy's sum does)
    :param center: optional approximate mean per variable.  Default (None): two passes, as the reference takes them -- the
        mean, then the squares of the differences from it.  With `center`: ONE pass over the data,
        mean = center + s1 / n and std = sqrt(s2 / n - (s1 / n)^2) from the sums of (x - center) and (x - center)^2; the
        subtraction cancels, so the std loses about 2 * log2(|mean - center| / std) bits when the center is far off
        (an exact center loses none).
    :return: (mean, std): two float64 numpy arrays over `axis`
    """
    with np.errstate(invalid='ignore', divide='ignore'):
        if center is None:
            m = _moments(array, axis, rows, None, skipna)
            mean = m[:, 1] / m[:, 0]
            m = _moments(array, axis, rows, mean, skipna)
            return mean, np.sqrt(m[:, 2] / m[:, 0])
        center = np.asarray(center, dtype=np.float64).reshape(-1)
        m = _moments(array, axis, rows, center, skipna)
        if m.shape[0] != center.size:
            raise ValueError('variable_statistics: center has %d entries, the array %d variables' % (center.size, m.shape[0]))
        r = m[:, 1] / m[:, 0]
        return center + r, np.sqrt(np.maximum(m[:, 2] / m[:, 0] - r * r, 0.0))


_LEADING_DIMS = ('f_hour', 'time', 'sample')


class VariableScaler(object):
    """
    The per-variable scaling of a predictor file: float32 `mean` / `std` tables over `dim` (the `mean` / `std` variables the
    reference writes over `varlev`, DLWP/model/preprocessing.py:687-700).  `transform` is `(x - mean) / std`
    (:660), `inverse_transform` is `x * std + mean` (Tutorial 4, cell 19): two rounded float32 operations per element on
    either side, so host and device results are the same bits.
    """

    def __init__(self, mean, std, dim='varlev'):
        self.mean = np.ascontiguousarray(np.asarray(mean, dtype=np.float32).reshape(-1))
        self.std = np.ascontiguousarray(np.asarray(std, dtype=np.float32).reshape(-1))
        self.dim = dim
        if self.mean.size != self.std.size:
            raise ValueError('VariableScaler: %d means and %d stds' % (self.mean.size, self.std.size))
        if not np.all(np.isfinite(self.std)) or np.any(self.std == 0):
            raise ValueError('VariableScaler: every std must be finite and non-zero as float32, got %s' % (self.std,))
        self._device = {}

    @classmethod
    def fit(cls, array, axis=1, rows=None, dim='varlev'):
        """the scaler of `variable_statistics(array, axis, rows)`"""
        mean, std = variable_statistics(array, axis=axis, rows=rows)
        return cls(mean, std, dim=dim)

    def __len__(self):
        return self.mean.size

    def sel(self, indices):
        """the scaler of a subset of the variables (a Generator's input / output selection applied to the tables)"""
        idx = np.asarray(indices)
        return VariableScaler(self.mean[idx], self.std[idx], dim=self.dim)

    def _tables(self, dev):
        key = str(dev)
        hit = self._device.get(key)
        if hit is None:
            import torch
            hit = (torch.from_numpy(self.mean).to(dev), torch.from_numpy(self.std).to(dev))
            self._device[key] = hit
        return hit

    # ------------------------------------------------------------------------------------------------------------- #
    def _axis(self, x, v, axis):
        if axis is None:
            axis = x.dims.index(self.dim) if hasattr(x, 'dims') else 1
        axis = axis % v.ndim
        if v.shape[axis] != len(self):
            raise ValueError('VariableScaler: axis %d of the array holds %d variables, the scaler %d'
                             % (axis, v.shape[axis], len(self)))
        return axis

    def _target(self, x, v, axis, channels_first):
        """position of the variable axis in the result"""
        if channels_first is False or channels_first is None:
            return axis
        if channels_first is not True:
            return int(channels_first) % v.ndim
        if hasattr(x, 'dims'):
            lead = [i for i, d in enumerate(x.dims) if d in _LEADING_DIMS and i != axis]
            return (max(lead) + 1 if lead else 0) - (1 if lead and axis < max(lead) else 0)
        return min(2, v.ndim - 1)

    def _apply(self, x, axis, out, inverse, channels_first=False):
        v = _raw(x)
        if not (isinstance(v, np.ndarray) or _is_tensor(v)):
            v = np.asarray(v)
        axis = self._axis(x, v, axis)
        pos = self._target(x, v, axis, channels_first)
        o = None if out is None else _raw(out)
        if _is_tensor(v) and v.is_cuda:
            res = self._apply_device(v, axis, pos, o, inverse)
        else:
            res = self._apply_host(v, axis, pos, o, inverse)
        if not hasattr(x, 'dims'):
            return res
        dims = list(x.dims)
        dims.insert(pos, dims.pop(axis))
        if out is x:
            x.values, x.dims = res, tuple(dims)
            return x
        return Forecast(res, dims, x.coords, getattr(x, 'name', 'forecast'))

    def _apply_host(self, v, axis, pos, o, inverse):
        if _is_tensor(v):
            v = v.detach().numpy()
        if o is not None and _is_tensor(o):
            o = o.detach().numpy()
        x = np.asarray(v, dtype=np.float32)
        shape = [1] * x.ndim
        shape[axis] = len(self)
        m, s = self.mean.reshape(shape), self.std.reshape(shape)
        target = tuple(np.moveaxis(np.empty(x.shape, dtype=np.bool_), axis, pos).shape) if pos != axis else x.shape
        if o is None:
            o = np.empty(target, dtype=np.float32)
        elif not isinstance(o, np.ndarray) or o.dtype != np.float32 or o.shape != target:
            raise ValueError('VariableScaler: out must be a float32 numpy array of shape %s' % (target,))
        ov = np.moveaxis(o, pos, axis) if pos != axis else o
        if inverse:
            np.multiply(x, s, out=ov)
            np.add(ov, m, out=ov)
        else:
            np.subtract(x, m, out=ov)
            np.divide(ov, s, out=ov)
        return o

    def _apply_device(self, v, axis, pos, o, inverse):
        import torch
        from .. import ops, _native as nat
        if v.dtype != torch.float32:
            raise TypeError('VariableScaler: device arrays must be float32, got %s' % v.dtype)
        mean_d, std_d = self._tables(v.device)
        target = list(v.shape)
        target.insert(pos, target.pop(axis))
        if o is None:
            o = torch.empty(target, dtype=torch.float32, device=v.device)
        elif not _is_tensor(o) or o.dtype != torch.float32 or o.device != v.device or list(o.shape) != target:
            raise ValueError('VariableScaler: out must be a float32 tensor of shape %s on %s' % (tuple(target), v.device))
        ov = o.movedim(pos, axis) if pos != axis else o
        mode = nat.AFFINE_MUL_ADD if inverse else nat.AFFINE_SUB_DIV
        try:
            ops.channel_affine(v, std_d, mean_d, mode, axis=axis, out=ov)
        except NotImplementedError:
            # a descriptor the library does not serve (more than nat.AFFINE_MAX_CHANNELS variables): the same two rounded
            # operations as torch expressions
            shape = [1] * v.dim()
            shape[axis] = len(self)
            m, s = mean_d.reshape(shape), std_d.reshape(shape)
            ov.copy_(v * s + m if inverse else (v - m) / s)
        return o

    def transform(self, x, axis=None, out=None):
        """
        (x - mean) / std along the variable axis.

        :param x: numpy array (host, float32 arithmetic), HIP tensor (float32, one launch; views are read through their
            strides where rows, variable axis and the merged rest describe them, otherwise copied first) or a `Forecast`
            whose values lie on either side (dims / coords are carried over)
        :param axis: int: the variable axis; default: the dim named `self.dim` of a Forecast, 1 for a plain array (the
            predictor layout (sample, varlev, ...))
        :param out: optional array of the result's shape and side; `out=x` scales in place
        """
        return self._apply(x, axis, out, False)

    def inverse_transform(self, x, axis=None, out=None, channels_first=False):
        """
        x * std + mean along the variable axis (Tutorial 4, cell 19).

        :param x, axis, out: as for `transform`
        :param channels_first: True: the result has the variable axis moved in front of the spatial dims -- behind the last
            of 'f_hour' / 'time' / 'sample' of a Forecast (('f_hour', 'time', 'varlev', 'x0', 'x1', 'x2'): cell 17's transpose),
            to position 2 of a plain array; an int: to that position.  On the device the layout changes in the same pass.
        """
        return self._apply(x, axis, out, True, channels_first)
