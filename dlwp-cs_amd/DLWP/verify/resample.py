"""
Sampling uncertainty of scores: the block bootstrap over initialisation times.  `bootstrap_mean` gives the replicate means of a
series of per-time score terms, `bootstrap_interval` percentile limits and a standard error for a mean, an RMSE, a ratio, an
anomaly correlation or a skill score built from such means, `bootstrap_difference` the paired comparison of two systems scored
on the same times.  Blocks of `block_length` consecutive times keep the serial correlation that `decorrelation_time` measures.

Values on a HIP device are resampled there (dlwpcs_row_resample: the series tile by tile in LDS, every resample served from the
tile) and every result stays there; numpy values take the float64 host twin `_resample_host`, the same sums in the same order
without the rounding to float32.  Neither falls back to the other.
"""
import numpy as np

from ..labelled import axis_of, device_scope, host as _host, is_tensor as _is_tensor, label, on_device as _on_device, raw as _raw
from .scores import _check_labels, _dev_operand
from .timeseries import _host_mean, _sqrt, _where_nan, effective_sample_size

_STATISTICS = {'mean': 1, 'rmse': 1, 'ratio': 2, 'correlation': 3, 'skill': 2}


class BootstrapInterval(object):
    """
    What `bootstrap_interval` and `bootstrap_difference` return.  `estimate` (the statistic of the whole sample), `low`, `high`
    (the percentile limits at (1 -+ level) / 2 of the replicates) and `standard_error` (the replicates' standard deviation, ddof
    1) are labelled like the input without the time dim; `level`, `n_resamples` and `block_length` are what was used;
    `replicates` (with the dim 'resample' where time stood) where asked for, else None; `p_value` from `bootstrap_difference`,
    else None.
    """
    __slots__ = ('estimate', 'low', 'high', 'standard_error', 'level', 'n_resamples', 'block_length', 'replicates', 'p_value')

    def __init__(self, estimate, low, high, standard_error, level, n_resamples, block_length, replicates=None, p_value=None):
        self.estimate, self.low, self.high, self.standard_error = estimate, low, high, standard_error
        self.level, self.n_resamples, self.block_length = float(level), int(n_resamples), int(block_length)
        self.replicates, self.p_value = replicates, p_value

    def __repr__(self):
        return 'BootstrapInterval(level=%g, n_resamples=%d, block_length=%d)' % (self.level, self.n_resamples, self.block_length)


def _int(v, lo, what, name):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < lo:
        raise ValueError('%s: %s must be an int of at least %d, got %r' % (name, what, lo, v))
    return int(v)


def bootstrap_starts(n_times, n_resamples=1000, block_length=1, circular=True, n_draw=None, seed=0):
    """
    The draw table of a block bootstrap: (n_resamples, nb) int32 block starts, nb = ceil(n_draw / block_length), uniform on
    0 .. n_times-1 (circular: a block that runs past the end wraps to the start) or on 0 .. n_times-block_length (moving blocks:
    none wraps), from `np.random.Generator(np.random.PCG64(seed))`: the same table for the same seed.  n_draw: the rows drawn
    per resample, default n_times; the last block is cut to fit.
    """
    name = 'bootstrap_starts'
    T = _int(n_times, 1, 'n_times', name)
    B = _int(n_resamples, 1, 'n_resamples', name)
    L = _int(block_length, 1, 'block_length', name)
    if L > T:
        raise ValueError('%s: block_length %d exceeds the %d times' % (name, L, T))
    nd = T if n_draw is None else _int(n_draw, 1, 'n_draw', name)
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.integers(0, T if circular else T - L + 1, size=(B, -(-nd // L)), dtype=np.int64).astype(np.int32)


def _resample_host(v, starts, block_length, n_draw=None, axis=0, propagate=False, min_count=1):
    """the definition of dlwpcs_row_resample in float64 on the host, without the rounding to float32: (values float64, int32
    counts), the resamples where `axis` stood.  A block's rows are added in row order from zero, the block sums in draw order."""
    x = np.moveaxis(np.asarray(v, dtype=np.float64), axis, 0)
    T, L = x.shape[0], int(block_length)
    nd = T if n_draw is None else int(n_draw)
    st = np.asarray(starts, dtype=np.int64)
    B, nb = st.shape
    ok = ~np.isnan(x)
    x0 = np.where(ok, x, 0.)
    drawn = (np.arange(nb)[:, None] * L + np.arange(L)[None, :]) < nd             # (nb, L): the last block is cut
    tail = (1,) * (x.ndim - 1)
    out = np.full((B,) + x.shape[1:], np.nan)
    cnt = np.zeros(out.shape, dtype=np.int32)
    need = nd if propagate else max(int(min_count), 1)
    zero = np.zeros((nb, 1) + x.shape[1:])
    with np.errstate(all='ignore'):
        for b in range(B):
            rows = (st[b][:, None] + np.arange(L)[None, :]) % T                    # (nb, L)
            m = drawn.reshape(drawn.shape + tail)
            vals = np.where(m, x0[rows], 0.)
            # (strictly sequential additions from zero: accumulate, never sum)
            blocks = np.add.accumulate(np.concatenate([zero, vals], axis=1), axis=1)[:, -1]
            tot = np.add.accumulate(np.concatenate([zero[:1, 0], blocks], axis=0), axis=0)[-1]
            n = (ok[rows] & m).sum(axis=(0, 1))
            cnt[b] = n
            out[b] = np.where(n >= need, tot / np.maximum(n, 1), np.nan)
    return np.moveaxis(out, 0, axis), np.moveaxis(cnt, 0, axis)


def _checks(level, missing, min_count, name):
    if level is not None and not (isinstance(level, (float, int, np.floating)) and 0. < float(level) < 1.):
        raise ValueError('%s: level must lie inside (0, 1), got %r' % (name, level))
    if missing not in ('propagate', 'skip'):
        raise ValueError("%s: 'missing' must be 'propagate' or 'skip'" % name)
    _int(min_count, 1, 'min_count', name)


def _components(x, name):
    comps = tuple(x) if isinstance(x, (tuple, list)) else (x,)
    if not comps:
        raise ValueError('%s: no series' % name)
    shape = tuple(_raw(comps[0]).shape)
    for c in comps[1:]:
        if tuple(_raw(c).shape) != shape:
            raise ValueError('%s: the component series %s and %s must have one shape' % (name, shape, tuple(_raw(c).shape)))
        if hasattr(c, 'dims') and hasattr(comps[0], 'dims'):
            _check_labels(comps[0], c)
    if len(shape) < 1:
        raise ValueError('%s: the series has no time axis' % name)
    return comps


def _operands(comps, name):
    """the values where they are resampled: all on the device when any is there (float32 there, nothing is converted), else all
    float64 on the host"""
    if _on_device(*comps):
        import torch
        for c in comps:
            r = _raw(c)
            if _is_tensor(r) and r.is_cuda and r.dtype != torch.float32:
                raise TypeError('%s: device values must be float32, got %s' % (name, r.dtype))
        with device_scope(*comps) as dev:
            return tuple(_dev_operand(c, dev) for c in comps)
    return tuple(np.asarray(_host(c), dtype=np.float64) for c in comps)


def _block_length(v, ax, block_length, name):
    """the block length as an int; 'auto': ceil(T / ESS) with ESS the median over the elements of effective_sample_size(v,
    method='ar1'), clipped to 1 .. T -- the one number that is downloaded"""
    T = int(v.shape[ax])
    if isinstance(block_length, str):
        if block_length != 'auto':
            raise ValueError("%s: block_length must be an int or 'auto', got %r" % (name, block_length))
        ess = effective_sample_size(v, method='ar1', axis=ax)
        if _is_tensor(ess):
            # the elements as the rows of one group of one column: the project's own quantile (NaN entries are no members, an empty
            # group gives NaN), any number of elements, nothing synchronises before the one download
            from .. import ops as dops
            rows = ess.reshape(-1, 1)
            n = int(rows.shape[0])
            med = float(dops.group_quantile(rows, [0, n], np.arange(n), [0.5], row_axis=0).item()) if n else float('nan')
        else:
            med = float(np.nanmedian(ess)) if np.any(~np.isnan(ess)) else float('nan')
        if not med == med:
            return 1
        return int(min(max(int(np.ceil(T / min(max(med, 1.), float(T)))), 1), T))
    L = _int(block_length, 1, 'block_length', name)
    if L > T:
        raise ValueError('%s: block_length %d exceeds the %d times' % (name, L, T))
    return L


def _draws(T, L, n_resamples, circular, seed, starts, name):
    nb = -(-T // L)
    if starts is None:
        return bootstrap_starts(T, n_resamples, L, circular, None, seed)
    if _is_tensor(starts):
        if tuple(starts.shape)[1:] != (nb,):
            raise ValueError('%s: starts %s must be (n_resamples, %d)' % (name, tuple(starts.shape), nb))
        return starts
    st = np.asarray(starts)
    if st.ndim != 2 or st.shape[0] < 1 or st.shape[1] != nb or st.dtype.kind not in 'iu':
        raise ValueError('%s: starts must be an (n_resamples, %d) array of ints, got %s %s' % (name, nb, st.shape, st.dtype))
    if st.min() < 0 or st.max() >= T:
        raise IndexError('%s: block start out of range of the %d times' % (name, T))
    return st.astype(np.int32)


def _resample(v, st, L, ax, missing, min_count):
    """(replicate means, counts) with the resamples at `ax`"""
    if _is_tensor(v):
        from .. import ops as dops
        return dops.row_resample(v, st, block_length=L, row_axis=ax, missing=missing, min_count=min_count, counts=True)
    if _is_tensor(st):
        st = st.detach().cpu().numpy()
    return _resample_host(v, st, L, None, ax, missing == 'propagate', min_count)


def _full_mean(v, ax, missing, min_count):
    """the mean of the whole sample, the time axis kept: the existing one-group group_mean on the device, the host mean else"""
    T = int(v.shape[ax])
    need = T if missing == 'propagate' else max(int(min_count), 1)
    if _is_tensor(v):
        from .. import ops as dops
        m, n = dops.group_mean(v, [0, T], np.arange(T), row_axis=ax, counts=True)
        return _where_nan(n < need, m)
    n = (~np.isnan(v)).sum(axis=ax, keepdims=True)
    return np.where(n >= need, _host_mean(v, ax), np.nan)


def _statistic(statistic, m, name):
    """the statistic elementwise on the means m (a tuple of arrays or tensors of one shape)"""
    if callable(statistic):
        return statistic(*m)
    with np.errstate(all='ignore'):
        if statistic == 'mean':
            return m[0]
        if statistic == 'rmse':
            return _sqrt(m[0])
        if statistic == 'ratio':
            return m[0] / m[1]
        if statistic == 'correlation':
            return m[0] / _sqrt(m[1] * m[2])
        return 1. - m[0] / m[1]


def _check_statistic(statistic, comps, name):
    if callable(statistic):
        return
    if not isinstance(statistic, str) or statistic not in _STATISTICS:
        raise ValueError("%s: statistic must be one of %s or a callable, got %r" % (name, ', '.join(sorted(_STATISTICS)), statistic))
    if len(comps) != _STATISTICS[statistic]:
        raise ValueError("%s: statistic '%s' takes %d component series, got %d" % (name, statistic, _STATISTICS[statistic], len(comps)))


def _spread(rep, ax, level):
    """(low, high, standard error) over the resample axis of the replicates, that axis dropped.  NaN replicates are left out."""
    B = int(rep.shape[ax])
    probs = [(1. - level) / 2., (1. + level) / 2.]
    if _is_tensor(rep):
        import torch
        from .. import ops as dops
        rep = rep.contiguous()
        q = dops.group_quantile(rep, [0, B], np.arange(B), probs, row_axis=ax)
        mean = dops.group_mean(rep, [0, B], np.arange(B), row_axis=ax)
        var, n = dops.time_lag(rep, None, lags=(0,), center_a=mean, row_axis=ax, counts=True)
        nf = n.to(torch.float32)
        se = _where_nan(n < 2, (var * (nf / (nf - 1.))).sqrt())
        return q[0].squeeze(ax), q[1].squeeze(ax), se.squeeze(ax)
    with np.errstate(all='ignore'):
        ok = ~np.isnan(rep)
        n = ok.sum(axis=ax)
        some = n > 0
        q = np.full((2,) + n.shape, np.nan)
        if np.any(some):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)
                q = np.nanquantile(rep, probs, axis=ax)
        dev = np.where(ok, rep - _host_mean(rep, ax), 0.)
        se = np.where(n >= 2, np.sqrt((dev * dev).sum(axis=ax) / np.maximum(n - 1, 1)), np.nan)
    return q[0], q[1], se


def _p_value(d, ax):
    """min(1, 2 min(frac(d <= 0), frac(d >= 0))) over the replicates that are not NaN; exact counts, one fp64 division"""
    if _is_tensor(d):
        import torch
        le, ge = (d <= 0).sum(dim=ax).double(), (d >= 0).sum(dim=ax).double()
        n = (~torch.isnan(d)).sum(dim=ax).double()
        p = torch.clamp(2. * torch.minimum(le, ge) / n, max=1.)
        return _where_nan(n < 1, p).to(torch.float32)
    with np.errstate(all='ignore'):
        le, ge = (d <= 0).sum(axis=ax).astype(np.float64), (d >= 0).sum(axis=ax).astype(np.float64)
        n = (~np.isnan(d)).sum(axis=ax).astype(np.float64)
        return np.where(n >= 1, np.minimum(2. * np.minimum(le, ge) / n, 1.), np.nan)


def _setup(comps, axis, n_resamples, block_length, circular, seed, starts, name):
    """(axis, values where they are resampled, L, draw table) for component series of one shape"""
    ax = axis_of(comps[0], 'time', explicit=axis)
    vals = _operands(comps, name)
    T = int(vals[0].shape[ax])
    if T < 1:
        raise ValueError('%s: the series has no times' % name)
    if starts is None:
        _int(n_resamples, 1, 'n_resamples', name)
    L = _block_length(vals[0], ax, block_length, name)
    return ax, vals, L, _draws(T, L, n_resamples, circular, seed, starts, name)


def bootstrap_mean(x, axis=None, n_resamples=1000, block_length=1, circular=True, seed=0, starts=None, missing='skip', min_count=1,
                   return_count=False):
    """
    The block-bootstrap replicates of the mean along time: per grid point and resample the mean over T times drawn with
    replacement in blocks of `block_length` consecutive times.

    :param x: a `Forecast` (or anything with `.dims`, `.coords`, `.values`), a numpy array or a torch tensor.  float32 values on
        a HIP device are resampled there (dlwpcs_row_resample: fp64 sums in a fixed order, rounded to float32 once) and the result
        stays there; numpy values are resampled on the host in float64 by the same rules
    :param axis: the time axis, a position or a dim name; None: the 'time' dim of a labelled input, else axis 0
    :param n_resamples, circular, seed: what `bootstrap_starts` draws the table from
    :param block_length: an int in 1 .. T, or 'auto': ceil(T / ESS) with ESS the median over the grid points of
        `effective_sample_size(x, method='ar1')`, clipped to 1 .. T; that median is one number downloaded from the device
    :param starts: a draw table of one's own, (n_resamples, ceil(T / block_length)) ints in 0 .. T-1 (IndexError outside); it
        outranks n_resamples, circular and seed
    :param missing: a NaN entry is missing.  'skip': a replicate is NaN where fewer than `min_count` of its draws are present;
        'propagate': where any is missing
    :param return_count: also return the int32 number of draws present
    :return: labelled like the input with the dim 'resample' where the time axis stood
    """
    name = 'bootstrap_mean'
    _checks(None, missing, min_count, name)
    comps = _components(x, name)
    if len(comps) != 1:
        raise ValueError('%s: one series, got %d' % (name, len(comps)))
    ax, vals, L, st = _setup(comps, axis, n_resamples, block_length, circular, seed, starts, name)
    out, cnt = _resample(vals[0], st, L, ax, missing, int(min_count))
    rows = {ax: ('resample', np.arange(int(st.shape[0]), dtype=np.int64))}
    res = label(comps[0], out, name, replace=rows)
    return (res, label(comps[0], cnt, name + '_count', replace=rows)) if return_count else res


def _replicates(statistic, vals, st, L, ax, missing, min_count, name):
    """(the statistic of the whole sample with the axis kept, the replicate statistics) of component values"""
    means = tuple(_resample(v, st, L, ax, missing, int(min_count))[0] for v in vals)
    full = tuple(_full_mean(v, ax, missing, min_count) for v in vals)
    return _statistic(statistic, full, name), _statistic(statistic, means, name)


def _record(src, ax, est, rep, level, L, B, return_replicates, name, p_value=None):
    low, high, se = _spread(rep, ax, level)
    est = est.squeeze(ax) if _is_tensor(est) else np.squeeze(est, axis=ax)
    lab = lambda v, what: label(src, v, name + '_' + what, drop=(ax,))       # noqa: E731
    reps = None
    if return_replicates:
        reps = label(src, rep, name + '_replicates', replace={ax: ('resample', np.arange(B, dtype=np.int64))})
    return BootstrapInterval(lab(est, 'estimate'), lab(low, 'low'), lab(high, 'high'), lab(se, 'standard_error'), level, B, L, reps,
                             None if p_value is None else lab(p_value, 'p_value'))


def bootstrap_interval(x, statistic='mean', level=0.95, axis=None, n_resamples=1000, block_length=1, circular=True, seed=0,
                       starts=None, missing='skip', min_count=1, return_replicates=False):
    """
    A block-bootstrap percentile interval for a statistic of means along time.

    :param x: one series of per-time terms, or a tuple of component series of one shape, all resampled with the SAME draw table
    :param statistic: with m1, m2, m3 the means of the components: 'mean' (m1), 'rmse' (sqrt m1 of a squared-error series),
        'ratio' (m1 / m2), 'correlation' (m1 / sqrt(m2 m3): the anomaly correlation from its three per-time sums), 'skill'
        (1 - m1 / m2), or a callable of the replicate means (arrays or device tensors), elementwise
    :param level: the coverage of the interval, inside (0, 1)
    :return: a `BootstrapInterval`: the estimate from the whole sample (the one-group `ops.group_mean` on the device), the limits
        at (1 -+ level) / 2 over the replicates (`ops.group_quantile` with one group of n_resamples rows on the device,
        `np.nanquantile` on the host), their standard deviation with ddof 1 (the lag-0 `ops.time_lag` on the device); every
        field labelled like the input without the time dim, on the device where the input is.  The other arguments are those of
        `bootstrap_mean`
    """
    name = 'bootstrap_interval'
    _checks(level, missing, min_count, name)
    comps = _components(x, name)
    _check_statistic(statistic, comps, name)
    ax, vals, L, st = _setup(comps, axis, n_resamples, block_length, circular, seed, starts, name)
    est, rep = _replicates(statistic, vals, st, L, ax, missing, min_count, name)
    return _record(comps[0], ax, est, rep, float(level), L, int(st.shape[0]), return_replicates, name)


def bootstrap_difference(a, b, statistic='mean', level=0.95, axis=None, n_resamples=1000, block_length=1, circular=True, seed=0,
                         starts=None, missing='skip', min_count=1, return_replicates=False):
    """
    The paired comparison of two systems scored on the same times: the replicates of statistic(a*) - statistic(b*), both drawn
    with one table, so that what the two share cancels.  a, b: what `bootstrap_interval` takes as x, of one shape;
    block_length='auto' is taken from a.

    :return: a `BootstrapInterval` of the difference, with `p_value` = min(1, 2 min(frac(d* <= 0), frac(d* >= 0))): the
        two-sided percentile test of "no difference"
    """
    name = 'bootstrap_difference'
    _checks(level, missing, min_count, name)
    ca, cb = _components(a, name), _components(b, name)
    _check_statistic(statistic, ca, name)
    if len(cb) != len(ca):
        raise ValueError('%s: the two systems have %d and %d component series' % (name, len(ca), len(cb)))
    _components(ca + cb, name)                                  # one shape, one set of labels
    ax, vals, L, st = _setup(ca + cb, axis, n_resamples, block_length, circular, seed, starts, name)
    ea, ra = _replicates(statistic, vals[:len(ca)], st, L, ax, missing, min_count, name)
    eb, rb = _replicates(statistic, vals[len(ca):], st, L, ax, missing, min_count, name)
    with np.errstate(all='ignore'):
        d, est = ra - rb, ea - eb
    return _record(ca[0], ax, est, d, float(level), L, int(st.shape[0]), return_replicates, name, _p_value(d, ax))
