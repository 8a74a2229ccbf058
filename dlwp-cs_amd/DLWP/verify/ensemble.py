"""
Ensemble scores of DLWP.verify: stacking forecasts along a member dim, mean, spread, CRPS, rank histograms.
"""
import numpy as np

from ..labelled import (axes as _axes, axis_of, coord, device_scope, Forecast, host as _host, is_tensor as _is_tensor, label,
                        on_device as _on_device, raw as _raw)
from .scores import _aligned_device, _bstrides, _check_labels, _dev_operand, _nanmean, _score_host, _weights

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
# the member axis: the dim named 'member' of a labelled input, which must have it, else `member_axis`
_MEMBER = dict(out_of_range='member_axis %d out of range of %d axes', missing="the ensemble's dims %s have no 'member'")


def _without_member(mx, elements=()):
    """the positions among the ensemble's dims that a result over its elements lacks: the member axis `mx`, and `elements`,
    which count the dims without it"""
    return (mx,) + tuple(a + (a >= mx) for a in elements)


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
                a, b = coord(ens, d), coord(valid, d)
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
    from .. import ops as dops
    with device_scope(ens, valid) as dev:
        et = _dev_operand(ens, dev)
        vt = _dev_operand(valid, dev) if valid is not None else None
        return dops.ensemble_stats(et, vt, member_axis=ax, want=want, fair=fair, ddof=ddof, variance=variance)


def ensemble_mean(ens, member_axis=0):
    """
    The mean over the members of every element.

    :param ens: ensemble: ndarray, device tensor, or a labelled array with a dim 'member' (`stack_forecasts`)
    :param member_axis: the member axis of an unlabelled input
    :return: the field without the member dim, labelled like the input, on the device when the input is; NaN where a member is
        NaN or infinite
    """
    ax = axis_of(ens, 'member', member_axis, **_MEMBER)
    _check_ensemble(ens, None, ax)
    return label(ens, _ensemble_fields(ens, None, ax, ('mean',))['mean'], 'ensemble_mean', drop=(ax,))


def ensemble_spread(ens, ddof=1, member_axis=0):
    """The standard deviation over the members of every element, sqrt(sum (x_i - mean)^2 / (M - ddof)); see `ensemble_mean`."""
    ax = axis_of(ens, 'member', member_axis, **_MEMBER)
    _check_ensemble(ens, None, ax)
    return label(ens, _ensemble_fields(ens, None, ax, ('spread',), ddof=ddof)['spread'], 'ensemble_spread', drop=(ax,))


def ensemble_crps(ens, valid, fair=False, member_axis=0):
    """
    The continuous ranked probability score of every element, mean_i |x_i - y| - sum_ij |x_i - x_j| / (2 M^2); fair=True divides
    the pair term by M (M - 1) instead (the score of the distribution the members were drawn from rather than of the M-member
    step function).  `valid` carries the dims of `ens` without the member dim (extents of 1 broadcast); a continuous series
    with one axis fewer raises NotImplementedError.  NaN where a member or the verification is NaN or infinite.
    """
    ax = axis_of(ens, 'member', member_axis, **_MEMBER)
    _check_ensemble(ens, valid, ax)
    return label(ens, _ensemble_fields(ens, valid, ax, ('crps',), fair=fair)['crps'], 'ensemble_crps', drop=(ax,))


def _field_mean(field, w, ax):
    """float64 nan-mean of field * w over the axes `ax` (numpy on the host, the score reduction on the device)"""
    if not _is_tensor(field):
        with np.errstate(invalid='ignore'):
            return np.asarray(_nanmean(field * (1. if w is None else w), ax), dtype=np.float64)
    from .. import ops as dops
    with device_scope(field) as dev:
        if w is not None:
            field = field * _dev_operand(w, dev)
        shape = tuple(int(e) for e in field.shape)
        out = dops.score_reduce('mean', [None, (field, _bstrides(field, shape)), None, None], shape, set(ax))
        return np.asarray(out.cpu().numpy(), dtype=np.float64)


def _mean_error(mean, valid, method, w, ax):
    """forecast_error's aligned form on the ensemble mean: the same code on either path"""
    if not _is_tensor(mean):
        return np.asarray(_score_host(method, mean, _host(valid), 0., 1. if w is None else w, ax), dtype=np.float64)
    with device_scope(mean) as dev:
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
    mx = axis_of(ens, 'member', member_axis, **_MEMBER)
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
    mx = axis_of(ens, 'member', member_axis, **_MEMBER)
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
    return label(ens, counts, 'rank_histogram', drop=_without_member(mx, ax), tail=[('rank', np.arange(M + 1))])
