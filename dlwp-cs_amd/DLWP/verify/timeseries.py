"""
Analysis along time in DLWP.verify: running means and Lanczos filters, least-squares fits (trends, harmonic climatologies),
Welch spectra and wavenumber-frequency diagrams, lagged covariances (autocorrelation, lead-lag maps, effective sample size).
"""
from collections import namedtuple

import numpy as np

from ..labelled import (axes as _axes, axis_of, coord, device_f32, device_scope, host as _host, is_tensor as _is_tensor, label,
                        on_device as _on_device, raw as _raw)
from .scores import _check_labels, _dev_operand
from .climatology import _lead_hours

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


def _time_filter_apply(x, h, axis, step, mode, mean, min_weight, relative, stamp, return_count, name):
    """`stamp`: the callers' `label=`, which row of a window gives an output its time coordinate"""
    if mode not in ('valid', 'same'):
        raise ValueError("'mode' must be 'valid' or 'same'")
    if stamp is None:
        stamp = 'end' if mode == 'valid' else 'centre'
    if stamp not in _FILTER_LABELS:
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
    rows = first + {'end': K - 1, 'centre': (K - 1) // 2, 'start': 0}[stamp]
    if hasattr(x, 'dims') and J and (rows[0] < 0 or rows[-1] >= T):
        raise ValueError("%s: label='%s' lies outside the series in mode '%s'" % (name, stamp, mode))
    if _on_device(v):
        from .. import ops as dops
        h32 = h.astype(np.float32)
        thr = np.float32(np.float32(min_weight) * _fp32_sum(h32)) if relative else np.float32(min_weight)
        with device_scope(v):
            res = dops.time_filter(device_f32(v), h, row_axis=axis, step=step, origin=origin, n_out=J, mode='mean' if mean else 'sum',
                                   min_weight=float(thr), counts=return_count)
        out, cnt = res if return_count else (res, None)
    else:
        tot = 0.
        for hk in h:
            tot = tot + hk
        thr = float(min_weight) * tot if relative else float(min_weight)
        out, cnt = _time_filter_host(_host(v), h, axis, step, origin, J, mean, thr)
    out = label(x, out, name, select={axis: rows}, lat=True)
    return (out, label(x, cnt, name + '_count', select={axis: rows}, lat=True)) if return_count else out


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
    return _time_filter_apply(x, weights, axis_of(x, 'time', explicit=axis), step, mode, missing == 'skip', min_weight, True, label, return_count,
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
    return _time_filter_apply(x, np.ones(n), axis_of(x, 'time', explicit=axis), step, mode, True, mc, False, label, return_count, 'running_mean')


def lead_window_mean(x, windows, axis=None, min_count=None):
    """
    Means over unequal windows of the lead axis (week 3, week 4, weeks 5 to 6 of a forecast): window i holds the rows
    windows[i][0] .. windows[i][1] - 1.  NaN entries are skipped; a window with fewer than `min_count` entries present (None:
    its length) is NaN.  axis=None: the 'f_hour' dim of a labelled input, else axis 0.  The coordinate of a window is that of
    its last row.  Device values are reduced there (dlwpcs_group_mean, fp64 sums), numpy values on the host in fp64.
    """
    axis = axis_of(x, 'f_hour', explicit=axis)
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
    if _on_device(v):
        import torch
        from .. import ops as dops
        with device_scope(v):
            out, cnt = dops.group_mean(device_f32(v), start, order, row_axis=axis, counts=True)
            need =torch.from_numpy(np.ascontiguousarray(mc.reshape(shape), dtype=np.int32)).to(v.device)
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
    return label(x, out, 'lead_window_mean', select={axis: win[:, 1] - 1}, lat=True)


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


def _fit(x, b32, axis, missing, min_count, return_count, name):
    if missing not in ('propagate', 'skip'):
        raise ValueError("'missing' must be 'propagate' or 'skip'")
    K = b32.shape[1]
    mc = K if min_count is None else int(min_count)
    if mc < K:
        raise ValueError('%s: min_count %d below the %d terms' % (name, mc, K))
    v = _raw(x)
    if _on_device(v):
        from .. import ops as dops
        with device_scope(v):
            res = dops.time_regression(device_f32(v), b32, row_axis=axis, missing=missing, min_count=mc, counts=return_count)
        coef, cnt = res if return_count else (res, None)
    else:
        coef, cnt = _time_regression_host(_host(v), b32, axis, missing == 'propagate', mc)
    out = label(x, coef, name, replace={axis: ('term', np.arange(K))}, lat=True)
    return (out, label(x, cnt, name + '_count', drop=(axis,), lat=True)) if return_count else out


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
    axis = axis_of(x, 'time', explicit=axis)
    b32 = _fit_basis32(basis, int(_raw(x).shape[axis]), 'time_regression')
    return _fit(x, b32, axis, missing, min_count, return_count, 'time_regression')


def _evaluate(coef, b32, term_axis, x, axis, name, rows_coord=None, row_dim='time'):
    """fitted values (x None) or residuals x - fitted, labelled"""
    c = _raw(coef)
    xv = None if x is None else _raw(x)
    if xv is not None and _on_device(xv) != _on_device(c):
        raise ValueError('%s: the data and the coefficients must both be on the device or both on the host' % name)
    if _on_device(c):
        from .. import ops as dops
        with device_scope(c):
            y = dops.time_regression_apply(device_f32(c), b32, src=None if xv is None else device_f32(xv), term_axis=term_axis,
                                           row_axis=axis)
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
        return label(x, y, name, lat=True)
    return label(coef, y, name, replace={term_axis: (row_dim, rows_coord)}, lat=True)


def regression_fitted(coef, basis, term_axis=None, times=None):
    """
    The fitted values sum_k basis[r, k] coef[k] of the coefficients of `time_regression` at the rows of `basis` (R, K; R need not
    be the length of the fit), in fp64 rounded to float32 once; NaN where the grid point's coefficients are.  A 'time' dim of R
    rows stands where the 'term' dim stood (its coordinate: `times`, when given).  Device coefficients are evaluated there.
    """
    term_axis = axis_of(coef, 'term', explicit=term_axis)
    b32 = _fit_basis32(basis, None, 'regression_fitted')
    if b32.shape[1] != int(_raw(coef).shape[term_axis]):
        raise ValueError('regression_fitted: %d coefficients, the basis has %d terms' % (_raw(coef).shape[term_axis], b32.shape[1]))
    return _evaluate(coef, b32, term_axis, None, term_axis, 'regression_fitted', None if times is None else np.asarray(times))


def regression_residual(x, coef, basis, axis=None, term_axis=None):
    """x minus the fitted values of `regression_fitted`, labelled like x: NaN where x or the grid point's coefficients are."""
    axis = axis_of(x, 'time', explicit=axis)
    term_axis = axis if term_axis is None and not hasattr(coef, 'dims') else axis_of(coef, 'term', explicit=term_axis)
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
    axis = axis_of(x, 'time', explicit=axis)
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
        axis = axis_of(self.coefficients, 'term')
        if f_hour is None:
            b32 = _fit_basis32(self.basis(t), None, 'harmonic_climatology')
            return _evaluate(self.coefficients, b32, axis, None, axis, 'climatology', t)
        when = t.astype('datetime64[s]')[None, :] + _lead_hours(f_hour).astype('timedelta64[s]')[:, None]
        b32 = _fit_basis32(self.basis(when.reshape(-1)), None, 'harmonic_climatology')
        flat = _evaluate(self.coefficients, b32, axis, None, axis, 'climatology', when.reshape(-1))
        v = _raw(flat)
        v = v.reshape(tuple(v.shape[:axis]) + when.shape + tuple(v.shape[axis + 1:]))
        v = v.movedim(axis, 0) if _is_tensor(v) else np.moveaxis(v, axis, 0)
        return label(flat, v, 'climatology', replace={axis: ('time', t)}, lead=[('f_hour', getattr(f_hour, 'values', f_hour))], lat=True)

    def anomalies(self, ds):
        axis = axis_of(ds, 'time')
        if not (hasattr(ds, 'coords') and 'time' in ds.coords):
            raise ValueError("harmonic_climatology: the data has no 'time' coordinate")
        b32 = _fit_basis32(self.basis(coord(ds, 'time')), int(_raw(ds).shape[axis]), 'harmonic_climatology')
        return _evaluate(self.coefficients, b32, axis_of(self.coefficients, 'term'), ds, axis, 'anomaly')


def harmonic_climatology(ds, n_harmonics=4, trend=False, min_count=None):
    """
    The harmonic climatology of a labelled series with a datetime64 'time' coordinate: a mean, with `trend` a linear trend, and
    `n_harmonics` harmonics of the tropical year, fitted per grid point to the rows that are not NaN (`time_regression`).  Where
    `daily_climatology` averages the thirty-odd values a day of the year has, this fits 1 + 2 n_harmonics numbers to all of them.
    Returns a `HarmonicClimatology`.
    """
    if not (hasattr(ds, 'dims') and 'time' in tuple(ds.dims) and 'time' in getattr(ds, 'coords', {})):
        raise ValueError("harmonic_climatology: the data needs a 'time' dimension with a coordinate")
    t = coord(ds, 'time')
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
    ax = axis_of(x, 'time', explicit=axis)
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


def _frequency(ax, K, M):
    """what stands at the time axis `ax` of a result (`label(replace=)`): 'frequency', K of them, in cycles per row"""
    return {ax: ('frequency', np.arange(K) / float(M))}


def _welch(a, b, n_segment, axis, hop, window, detrend, n_freq, min_count, name):
    """(quantities (nq, ...), counts, axis, what stands there in the result (`_frequency`)): numpy float64 for host values, float32
    device tensors for device values"""
    if b is not None:
        _check_labels(a, b)
        if tuple(_raw(a).shape) != tuple(_raw(b).shape):
            raise ValueError('%s: the two series %s and %s must have one shape' % (name, tuple(_raw(a).shape), tuple(_raw(b).shape)))
    ax, M, hop, w, sw, dt, K, mc = _welch_args(a, n_segment, axis, hop, window, detrend, n_freq, min_count, name)
    if _on_device(a, b):
        from .. import ops as dops
        with device_scope(a, b) as dev:
            at = _dev_operand(a, dev)
            bt = _dev_operand(b, dev) if b is not None else None
            out, cnt = dops.time_spectrum(at, bt, n_segment=M, hop=hop, window=w, row_axis=ax, detrend=dt, n_freq=K, min_count=mc,
                                          counts=True)
        return (out if b is not None else out[None]), cnt, ax, _frequency(ax, K, M)
    out, cnt = _welch_host(_host(a), None if b is None else _host(b), ax, M, hop, w, sw, dt, K, mc)
    return out, cnt, ax, _frequency(ax, K, M)


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
    out, cnt, ax, freq = _welch(x, None, n_segment, axis, hop, window, detrend, n_freq, min_count, 'time_spectrum')
    res = label(x, out[0], 'time_spectrum', replace=freq, lat=True)
    return (res, label(x, cnt, 'time_spectrum_count', drop=(ax,))) if return_count else res


def time_cross_spectrum(a, b, n_segment, axis=None, hop=None, window='hann', detrend='constant', n_freq=None, min_count=1,
                        return_count=False):
    """
    The power spectra of two series of one shape and their cross-spectrum along time, averaged over the segments that are finite
    in both: TimeCrossSpectrum(power_a, power_b, co, quad) with co + i quad = c_f A_f conj(B_f) / (M S_w).  Arguments as for
    `time_spectrum`.
    """
    out, cnt, ax, freq = _welch(a, b, n_segment, axis, hop, window, detrend, n_freq, min_count, 'time_cross_spectrum')
    res = TimeCrossSpectrum(*[label(a, out[i], n, replace=freq, lat=True) for i, n in enumerate(TimeCrossSpectrum._fields)])
    return (res, label(a, cnt, 'time_cross_spectrum_count', drop=(ax,))) if return_count else res


def time_coherence(a, b, n_segment, axis=None, hop=None, window='hann', detrend='constant', n_freq=None, min_count=1,
                   return_count=False):
    """
    Squared coherence (co^2 + quad^2) / (power_a power_b) per frequency, formed from the segment-AVERAGED spectra of
    `time_cross_spectrum` (per segment it would be identically 1): 1 where the forecast holds the verification's phase over the
    segments, near 1 / segments where the two are unrelated.  NaN where either power is 0.  Arguments as for `time_spectrum`.
    """
    out, cnt, ax, freq = _welch(a, b, n_segment, axis, hop, window, detrend, n_freq, min_count, 'time_coherence')
    if _is_tensor(out):
        den = out[0] * out[1]
        coh = (out[2] ** 2 + out[3] ** 2) / den
        coh = coh.masked_fill(den == 0, float('nan'))
    else:
        with np.errstate(invalid='ignore', divide='ignore'):
            coh = np.where(out[0] * out[1] == 0, np.nan, (out[2] ** 2 + out[3] ** 2) / (out[0] * out[1]))
    res = label(a, coh, 'time_coherence', replace=freq, lat=True)
    return (res, label(a, cnt, 'time_coherence_count', drop=(ax,))) if return_count else res


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
    if _on_device(v):
        import torch
        from .. import ops as dops
        with device_scope(v):
            z = dops.time_fourier(device_f32(v), n_segment=M, hop=hop, window=w, row_axis=ax, detrend=dt, n_freq=K)
            out = torch.view_as_complex(z.movedim(ax + 2, -1).contiguous())
    else:
        X, _ = _fourier_host(np.moveaxis(np.asarray(_host(v), dtype=np.float64), ax, 0), M, hop, w, dt, K)
        out = np.moveaxis(X, 1, ax + 1)
    if n_segment is None:
        return label(x, out[0], 'time_fourier', replace=_frequency(ax, K, M), lat=True)
    return label(x, out, 'time_fourier', replace=_frequency(ax, K, M), lead=[('segment', None)], lat=True)


def _mirror(x, lat_axis, component, name):
    """(x + flip) / 2 or (x - flip) / 2 along lat_axis: the part symmetric or antisymmetric about the equator"""
    if component not in ('symmetric', 'antisymmetric'):
        raise ValueError("%s: 'component' must be None, 'symmetric' or 'antisymmetric'" % name)
    if lat_axis is None:
        raise ValueError('%s: a component needs a latitude axis' % name)
    if hasattr(x, 'coords') and hasattr(x, 'dims') and x.dims[lat_axis] in x.coords:
        lat = np.asarray(coord(x, x.dims[lat_axis]), dtype=np.float64)
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
    ax = axis_of(x, 'time', explicit=axis)
    lon = axis_of(x, 'lon', lon_axis, 'lon_axis %d out of range of %d axes')
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
    if _on_device(v):
        import torch
        from .. import ops as dops
        with device_scope(v):
            z = dops.time_fourier(device_f32(v), row_axis=lon, n_freq=Kw)[0].movedim(lon + 1, -1)     # (..., wavenumber, ..., 2)
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
    wave = {lon: ('wavenumber', np.arange(Kw))}
    ren = {**wave, **_frequency(ax, K, M)}
    res = WavenumberFrequencySpectrum(label(x, east, 'eastward', replace=ren, lat=True), label(x, west, 'westward', replace=ren, lat=True))
    return (res, label(x, cnt, name + '_count', drop=(ax,), replace=wave)) if return_count else res


# --------------------------------------------------------------------------------------------------------------------- #
# Lagged covariances along time: lead-lag maps, autocorrelation, decorrelation time, effective sample size
# --------------------------------------------------------------------------------------------------------------------- #
#
# Lag l pairs a[t] with b[t + l]: a positive lag means that a leads.  c_l is the mean over the pairs present (neither entry NaN) of
# (a[t] - mean a) (b[t + l] - mean b), the means taken once over the rows present of each series.  numpy values go through
# _time_lag_host in float64, device tensors through dlwpcs_time_lag (fp32 deviations, exact fp64 products in a fixed order) after
# one group_mean pass per operand for the means, and stay on the device as float32; neither path falls back to the other.  The
# new dim is 'lag', in rows.

_LAG_MAX = 1024


def _lag_list(lags, auto, name):
    """the lags as int64: an int L means 0 .. L (auto) or -L .. L; a sequence must be an ascending arithmetic progression"""
    if isinstance(lags, (int, np.integer)) and not isinstance(lags, bool):
        if int(lags) < 0:
            raise ValueError('%s: a largest lag of %d' % (name, lags))
        lg = np.arange(0 if auto else -int(lags), int(lags) + 1, dtype=np.int64)
    else:
        lg = np.asarray(lags)
        if lg.ndim != 1 or lg.size < 1 or lg.dtype.kind not in 'iu':
            raise ValueError('%s: lags must be an int or a non-empty sequence of ints, got %r' % (name, lags))
        lg = lg.astype(np.int64)
        if lg.size > 1 and (lg[1] - lg[0] < 1 or np.any(np.diff(lg) != lg[1] - lg[0])):
            raise ValueError('%s: lags must be an ascending arithmetic progression, got %r' % (name, lags))
    if lg.size > _LAG_MAX:
        raise ValueError('%s: %d lags (1 .. %d)' % (name, lg.size, _LAG_MAX))
    return lg


def _lag_form(a, b, ax, name):
    if b is None:
        return 'auto'
    sa, sb = tuple(_raw(a).shape), tuple(_raw(b).shape)
    if sa == sb:
        if hasattr(b, 'dims'):
            _check_labels(a, b)
        return 'pair'
    if len(sb) == 1 and sb[0] == sa[ax]:
        return 'index'
    raise ValueError('%s: the second series %s must have the shape of the first %s or be a vector of its %d rows' % (name, sb, sa, sa[ax]))


def _lag_checks(center, missing, min_count, name):
    if center not in ('mean', None):
        raise ValueError("%s: 'center' must be 'mean' or None" % name)
    if missing not in ('propagate', 'skip'):
        raise ValueError("%s: 'missing' must be 'propagate' or 'skip'" % name)
    if int(min_count) < 1:
        raise ValueError('%s: min_count must be at least 1, got %d' % (name, min_count))


def _time_lag_host(a, b, lags, axis, center_a=None, center_b=None, propagate=False, min_count=1):
    """the definition of dlwpcs_time_lag in float64 on the host: (values float64, int32 counts), the lags where `axis` stood.  b:
    None, an array of a's shape or a vector of its rows; the centres broadcast against the operands moved to rows first."""
    va = np.moveaxis(np.asarray(a, dtype=np.float64), axis, 0)
    T, tail = va.shape[0], (None,) * (va.ndim - 1)
    if b is None:
        vb, center_b = va, center_a if center_b is None else center_b
    else:
        vb = np.asarray(b, dtype=np.float64)
        vb = vb[(slice(None),) + tail] if vb.ndim == 1 and va.ndim > 1 else np.moveaxis(vb, axis, 0)
    pa, pb = ~np.isnan(va), ~np.isnan(vb)
    with np.errstate(all='ignore'):
        da = np.where(pa, va - (0. if center_a is None else center_a), 0.)
        db = np.where(pb, vb - (0. if center_b is None else center_b), 0.)
        out = np.full((len(lags),) + va.shape[1:], np.nan)
        cnt = np.zeros(out.shape, dtype=np.int32)
        for i, l in enumerate(int(x) for x in lags):
            t0, t1 = max(0, -l), min(T, T - l)
            if t1 <= t0:
                continue
            s = (da[t0:t1] * db[t0 + l:t1 + l]).sum(axis=0)
            n = (pa[t0:t1] & pb[t0 + l:t1 + l]).sum(axis=0)
            need = max(T - abs(l), 1) if propagate else max(int(min_count), 1)
            cnt[i] = n
            out[i] = np.where(n >= need, s / np.maximum(n, 1), np.nan)
    return np.moveaxis(out, 0, axis), np.moveaxis(cnt, 0, axis)


def _host_mean(v, axis):
    """the mean over the rows present, axis kept: float64"""
    ok = ~np.isnan(v)
    n = ok.sum(axis=axis, keepdims=True)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(n > 0, np.where(ok, v, 0.).sum(axis=axis, keepdims=True) / np.maximum(n, 1), np.nan)


def _dev_mean(t, axis):
    """the mean over the rows present on the device, axis kept: ops.group_mean with one group, the fp64 sum rounded to fp32 once"""
    from .. import ops as dops
    T = int(t.shape[axis])
    if T == 0:
        return None
    return dops.group_mean(t, [0, T], np.arange(T), row_axis=axis)


def _lag_run(a, b, form, lags, ax, center, missing, min_count):
    """(values, counts) with the lags at `ax`: float32 / int32 device tensors for device values, float64 / int32 numpy otherwise"""
    if _on_device(a, b):
        from .. import ops as dops
        with device_scope(a, b) as dev:
            at = _dev_operand(a, dev)
            bt = None if b is None else _dev_operand(b, dev)
            ca = _dev_mean(at, ax) if center else None
            cb = None
            if center and bt is not None:
                cb = _dev_mean(bt, 0 if form == 'index' else ax)
            return dops.time_lag(at, bt, lags=lags, center_a=ca, center_b=cb, row_axis=ax, missing=missing, min_count=min_count,
                                 counts=True)
    ha = np.asarray(_host(a), dtype=np.float64)
    hb = None if b is None else np.asarray(_host(b), dtype=np.float64)
    ca = cb = None
    if center:
        ca = np.moveaxis(_host_mean(ha, ax), ax, 0)
        if hb is not None:
            cb = _host_mean(hb, 0) if form == 'index' else np.moveaxis(_host_mean(hb, ax), ax, 0)
    return _time_lag_host(ha, hb, lags, ax, ca, cb, missing == 'propagate', min_count)


def _lag_operands(a, b):
    """the values of the two series where they are reduced: both on the device when either is there, else both on the host"""
    if _on_device(a, b):
        with device_scope(a, b) as dev:
            return _dev_operand(a, dev), None if b is None else _dev_operand(b, dev)
    return _host(a), None if b is None else _host(b)


def _take(v, ax, i):
    """row i of axis ax, the axis kept"""
    return v.narrow(ax, i, 1) if _is_tensor(v) else np.take(v, [i], axis=ax)


def _where_nan(cond, v):
    """v with NaN where cond"""
    if _is_tensor(v):
        return v.masked_fill(cond, float('nan'))
    return np.where(cond, np.nan, v)


def _sqrt(v):
    if _is_tensor(v):
        return v.sqrt()
    with np.errstate(invalid='ignore'):
        return np.sqrt(v)


def _ratio(num, den):
    """num / den, NaN where den is not positive"""
    if _is_tensor(num):
        return _where_nan(~(den > 0), num / den)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(den > 0, num / den, np.nan)


def _lag_label(src, values, name, ax, lags):
    return label(src, values, name, replace={ax: ('lag', np.asarray(lags, dtype=np.int64))}, lat=True)


def _variance0(x, ax, center, missing, min_count):
    """the lag-0 autocovariance of x, the lag axis kept: one one-lag auto call"""
    return _lag_run(x, None, 'auto', np.zeros(1, np.int64), ax, center, missing, min_count)[0]


def lag_covariance(a, b=None, lags=0, axis=None, center='mean', missing='skip', min_count=1, norm='pairs', return_count=False):
    """
    The lagged covariance along time, per grid point and lag l: the mean over the pairs present of (a[t] - mean a)
    (b[t + l] - mean b).  A positive lag means that a leads.

    :param a: a `Forecast` (or anything with `.dims`, `.coords`, `.values`), a numpy array or a torch tensor.  Values on a HIP
        device are reduced there (dlwpcs_time_lag: fp32 deviations, exact fp64 products in a fixed order) and the float32 result
        stays there; numpy values are reduced on the host in float64 by the same rules
    :param b: None (the autocovariance of a), a series of a's shape, or a vector of T values shared by every grid point (an index)
    :param lags: an int L: the lags 0 .. L (b=None) or -L .. L; or ints in an ascending arithmetic progression (at most 1024).
        A lag beyond the series has no pairs
    :param axis: the time axis, a position or a dim name; None: the 'time' dim of a labelled input, else axis 0
    :param center: 'mean': each series loses its mean over the rows present, taken once over the whole series (on the device the
        fp64 sum rounded to float32 once); None: nothing is subtracted
    :param missing: a NaN entry is missing.  'skip': a lag is NaN where fewer than `min_count` pairs are present; 'propagate':
        where any pair inside the series has a missing entry
    :param norm: 'pairs': the sum over the n_l pairs present divided by n_l.  'biased': divided by n_0 instead (the estimator
        whose autocovariance matrix is positive semi-definite); it needs lag 0 among the lags
    :param return_count: also return the int32 number of pairs present per lag
    :return: labelled like the input with the dim 'lag' (rows) where the time axis stood
    """
    name = 'lag_covariance'
    ax = axis_of(a, 'time', explicit=axis)
    _lag_checks(center, missing, min_count, name)
    if norm not in ('pairs', 'biased'):
        raise ValueError("%s: 'norm' must be 'pairs' or 'biased'" % name)
    form = _lag_form(a, b, ax, name)
    lg = _lag_list(lags, form == 'auto', name)
    if norm == 'biased' and 0 not in lg:
        raise ValueError("%s: norm='biased' needs lag 0 among the lags" % name)
    out, cnt = _lag_run(a, b, form, lg, ax, center, missing, int(min_count))
    if norm == 'biased':
        n0 = _take(cnt, ax, int(np.flatnonzero(lg == 0)[0]))
        if _is_tensor(out):
            out = out * (cnt.to(out.dtype) / n0.to(out.dtype))
        else:
            with np.errstate(invalid='ignore', divide='ignore'):
                out = out * (cnt / n0.astype(np.float64))
    res = _lag_label(a, out, name, ax, lg)
    return (res, _lag_label(a, cnt, name + '_count', ax, lg)) if return_count else res


def _correlation(a, b, lags, axis, center, missing, min_count, name):
    """(correlations, counts, axis, lags) of lag_correlation"""
    ax = axis_of(a, 'time', explicit=axis)
    _lag_checks(center, missing, min_count, name)
    form = _lag_form(a, b, ax, name)
    lg = _lag_list(lags, form == 'auto', name)
    mc = int(min_count)
    va_, vb_ = _lag_operands(a, b)
    out, cnt = _lag_run(va_, vb_, form, lg, ax, center, missing, mc)
    if form == 'auto':
        at0 = np.flatnonzero(lg == 0)
        v0 = _take(out, ax, int(at0[0])) if at0.size else _variance0(va_, ax, center, missing, mc)
        return _ratio(out, v0), cnt, ax, lg
    var_a = _variance0(va_, ax, center, missing, mc)
    var_b = _variance0(vb_, 0, center, missing, mc).reshape(()) if form == 'index' else _variance0(vb_, ax, center, missing, mc)
    return _ratio(out, _sqrt(var_a) * _sqrt(var_b)), cnt, ax, lg


def lag_correlation(a, b=None, lags=0, axis=None, center='mean', missing='skip', min_count=1, return_count=False):
    """
    The lagged correlation c_l / sqrt(c_aa(0) c_bb(0)) along time, c_l the covariance of `lag_covariance` (norm='pairs') and
    c_aa(0), c_bb(0) the lag-0 autocovariances of the two series over their own rows present.  b=None: the autocorrelation, c_l
    divided by lag 0 of the same call (where lag 0 is not among the lags it is computed by one more one-lag call and not
    returned).  With a second series the two variances are two more one-lag calls, each with its own pass for the mean: on the
    device that is four extra passes over the data.  NaN where a variance is not positive.  Arguments as for `lag_covariance`.
    """
    out, cnt, ax, lg = _correlation(a, b, lags, axis, center, missing, min_count, 'lag_correlation')
    res = _lag_label(a, out, 'lag_correlation', ax, lg)
    return (res, _lag_label(a, cnt, 'lag_correlation_count', ax, lg)) if return_count else res


def autocorrelation(x, max_lag, axis=None, center='mean', missing='skip', min_count=1, return_count=False):
    """The autocorrelation function r_0 .. r_max_lag of a series along time: `lag_correlation` of x with itself (r_0 = 1 where
    the variance is positive)."""
    if not isinstance(max_lag, (int, np.integer)) or isinstance(max_lag, bool) or int(max_lag) < 0:
        raise ValueError('autocorrelation: max_lag must be an int of at least 0, got %r' % (max_lag,))
    out, cnt, ax, lg = _correlation(x, None, int(max_lag), axis, center, missing, min_count, 'autocorrelation')
    res = _lag_label(x, out, 'autocorrelation', ax, lg)
    return (res, _lag_label(x, cnt, 'autocorrelation_count', ax, lg)) if return_count else res


def lag_regression(index, x, lags=0, axis=None, center='mean', missing='skip', min_count=1, return_correlation=False):
    """
    Lead-lag regression maps of a field onto an index: per grid point and lag l the slope cov(index[t], x[t + l]) / var(index),
    what the field looks like l rows after (l < 0: before) the index peaks by one unit.

    :param index: a (T,) series on the host or the device, e.g. one principal component of `eof_analysis`
    :param x: the field, T rows along time; device values are reduced there (the index is uploaded where it is not)
    :param lags: an int L: -L .. L; or ints in an ascending arithmetic progression
    :param return_correlation: also return the correlation maps cov / sqrt(var(index) var(x)), var(x) by one more one-lag call
    Other arguments as for `lag_covariance`.  Labelled like x with the dim 'lag' where the time axis stood.
    """
    name = 'lag_regression'
    ax = axis_of(x, 'time', explicit=axis)
    _lag_checks(center, missing, min_count, name)
    iv = _raw(index)
    T = int(_raw(x).shape[ax])
    if len(iv.shape) != 1 or int(iv.shape[0]) != T:
        raise ValueError('%s: the index %s must be a vector of the %d rows of the data' % (name, tuple(iv.shape), T))
    lg = _lag_list(lags, False, name)
    mc = int(min_count)
    # the kernel pairs x[s] with index[s + k]: k = -l, so the lags run backwards and the result is turned round
    xv, iv = _lag_operands(x, iv)
    out, _ = _lag_run(xv, iv, 'index', -lg[::-1], ax, center, missing, mc)
    out = out.flip(ax) if _is_tensor(out) else np.flip(out, ax)
    vi = _variance0(iv, 0, center, missing, mc).reshape(())
    slope = _lag_label(x, _ratio(out, vi), name, ax, lg)
    if not return_correlation:
        return slope
    vx = _variance0(xv, ax, center, missing, mc)
    corr = _lag_label(x, _ratio(out, _sqrt(vi) * _sqrt(vx)), name + '_correlation', ax, lg)
    return slope, corr


def decorrelation_time(x, max_lag, threshold=float(np.exp(-1.)), axis=None, center='mean', missing='skip', min_count=1):
    """
    The e-folding time of a series along time, in rows: the first crossing of the autocorrelation r_0 .. r_max_lag below
    `threshold`, linearly interpolated between the two lags around it; inf where it never crosses within max_lag, NaN where the
    autocorrelation is NaN before it crosses.  The time axis is dropped.
    """
    name = 'decorrelation_time'
    if not isinstance(max_lag, (int, np.integer)) or isinstance(max_lag, bool) or int(max_lag) < 1:
        raise ValueError('%s: max_lag must be an int of at least 1, got %r' % (name, max_lag))
    if not 0. < float(threshold) < 1.:
        raise ValueError('%s: a threshold of %r is outside (0, 1)' % (name, threshold))
    r, _, ax, lg = _correlation(x, None, int(max_lag), axis, center, missing, min_count, name)
    thr = float(threshold)
    if _is_tensor(r):
        import torch
        r = r.movedim(ax, 0)
        below = r[1:] < thr
        bad = torch.isnan(r).cumsum(0)[1:] > 0                               # a NaN at or before this lag
        k = (below | bad).to(torch.int8).argmax(0, keepdim=True)              # the first such lag is k + 1
        hi, lo = r[:-1].gather(0, k)[0], r[1:].gather(0, k)[0]
        tau = k[0].to(r.dtype) + (hi - thr) / (hi - lo)
        tau = torch.where(below.any(0) | bad.any(0), tau, torch.full_like(tau, float('inf')))
        tau = _where_nan(bad.gather(0, k)[0] | torch.isnan(r[0]), tau)
    else:
        r = np.moveaxis(r, ax, 0)
        below = r[1:] < thr
        bad = np.cumsum(np.isnan(r), axis=0)[1:] > 0
        k = np.argmax(below | bad, axis=0)[None]
        hi, lo = np.take_along_axis(r[:-1], k, 0)[0], np.take_along_axis(r[1:], k, 0)[0]
        with np.errstate(invalid='ignore', divide='ignore'):
            tau = k[0] + (hi - thr) / (hi - lo)
        tau = np.where(below.any(0) | bad.any(0), tau, np.inf)
        tau = np.where(np.take_along_axis(bad, k, 0)[0] | np.isnan(r[0]), np.nan, tau)
    return label(x, tau, name, drop=(ax,), lat=True)


def effective_sample_size(x, b=None, method='ar1', max_lag=None, axis=None, center='mean', missing='skip', min_count=1):
    """
    The effective number of independent samples of a series along time (of the pair x, b for the significance of their
    correlation), with n the rows present (pair: present in both) and r_k the autocorrelations (pair: the products r_k(x) r_k(b)):
    method='ar1': n (1 - r_1) / (1 + r_1) (Bretherton et al. 1999); method='sum': n / (1 + 2 sum_{k=1..max_lag} (1 - k / n) r_k).
    Clipped to [1, n]; NaN where an autocorrelation is.  The time axis is dropped.
    """
    name = 'effective_sample_size'
    if method not in ('ar1', 'sum'):
        raise ValueError("%s: 'method' must be 'ar1' or 'sum'" % name)
    if method == 'sum':
        if not isinstance(max_lag, (int, np.integer)) or isinstance(max_lag, bool) or int(max_lag) < 1:
            raise ValueError("%s: method='sum' needs max_lag, an int of at least 1, got %r" % (name, max_lag))
    elif max_lag is not None:
        raise ValueError("%s: max_lag belongs to method='sum'" % name)
    K = 1 if method == 'ar1' else int(max_lag)
    ax = axis_of(x, 'time', explicit=axis)
    if b is not None and tuple(_raw(b).shape) != tuple(_raw(x).shape):
        raise ValueError('%s: the two series %s and %s must have one shape' % (name, tuple(_raw(x).shape), tuple(_raw(b).shape)))
    xv, bv = _lag_operands(x, b)
    r, cnt, _, lg = _correlation(xv, None, K, ax, center, missing, min_count, name)
    n = _take(cnt, ax, 0)
    if bv is not None:
        r = r * _correlation(bv, None, K, ax, center, missing, min_count, name)[0]
        n = _take(_lag_run(xv, bv, 'pair', np.zeros(1, np.int64), ax, None, missing, int(min_count))[1], ax, 0)
    tensor = _is_tensor(r)
    nf = n.to(r.dtype) if tensor else n.astype(np.float64)
    shape = [1] * len(r.shape)
    shape[ax] = K
    k = np.arange(1, K + 1, dtype=np.float64).reshape(shape)
    if tensor:
        import torch
        k = torch.from_numpy(k).to(r.device, r.dtype)
    rk = r.narrow(ax, 1, K) if tensor else np.take(r, np.arange(1, K + 1), axis=ax)
    with np.errstate(invalid='ignore', divide='ignore'):
        if method == 'ar1':
            ess = nf * (1. - rk) / (1. + rk)
        else:
            terms = (1. - k / nf) * rk
            ess = nf / (1. + 2. * (terms.sum(ax, keepdim=True) if tensor else terms.sum(axis=ax, keepdims=True)))
    if tensor:
        import torch
        nan = torch.isnan(ess)
        ess = _where_nan(nan | (nf < 1), torch.minimum(torch.maximum(ess, torch.ones_like(ess)), nf))
        ess = ess.squeeze(ax)
    else:
        with np.errstate(invalid='ignore'):
            ess = np.where(np.isnan(ess) | (nf < 1), np.nan, np.minimum(np.maximum(ess, 1.), nf))
        ess = np.squeeze(ess, axis=ax)
    return label(x, ess, name, drop=(ax,), lat=True)
