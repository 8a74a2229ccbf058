"""
Categorical probability scores of an ensemble in DLWP.verify: probabilities, Brier and ranked probability scores, reliability
counts.
"""
import numpy as np

from ..labelled import (axes as _axes, axis_of, coord, device_scope, host as _host, is_tensor as _is_tensor, label,
                        on_device as _on_device)
from .scores import _dev_operand, _weights
from .climatology import ClimatologyLookup
from .ensemble import _MEMBER, _check_ensemble, _field_mean, _without_member

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
    """(thresholds, their threshold axis, Q, dim name, its coordinate (arange(Q) where it has none)): the threshold dim is 'quantile' or 'threshold' of a
    labelled input, else `threshold_axis`; the other dims must be those of the ensemble without the member dim (extents of 1
    broadcast), or there are none (a bare vector).  A ClimatologyLookup is laid out first."""
    if isinstance(thresholds, ClimatologyLookup):
        thresholds = thresholds.materialize()
    if not hasattr(thresholds, 'shape'):
        thresholds = np.asarray(thresholds, dtype=np.float64)
    shape = tuple(int(e) for e in thresholds.shape)
    name, tcoord = 'threshold', None
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
            tcoord = coord(thresholds, name)
        if hasattr(ens, 'dims') and len(td) > 1:
            ed = tuple(d for d in ens.dims if d != 'member')
            if td[:ta] + td[ta + 1:] != ed:
                raise ValueError("the thresholds' dims %s without '%s' do not match the ensemble dims %s without the member dim"
                                 % (td, name, tuple(ens.dims)))
    else:
        ta = axis_of(thresholds, None, threshold_axis, 'threshold_axis %d out of range of %d axes')
    eshape = tuple(int(e) for i, e in enumerate(ens.shape) if i != mx)
    if len(shape) > 1:
        rest = shape[:ta] + shape[ta + 1:]
        if len(rest) != len(eshape) or any(t not in (1, e) for t, e in zip(rest, eshape)):
            raise ValueError('the thresholds %s without their threshold axis must carry the dims of the ensemble without the '
                             'member dim %s (extents of 1 broadcast)' % (shape, eshape))
    if shape[ta] < 1:
        raise ValueError('at least one threshold is needed')
    return thresholds, ta, shape[ta], name, np.arange(shape[ta]) if tcoord is None else tcoord


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
    from .. import ops as dops
    with device_scope(ens, valid, thresholds) as dev:
        et, tt =_dev_operand(ens, dev), _dev_operand(thresholds, dev)
        vt = _dev_operand(valid, dev) if valid is not None else None
        return dops.ensemble_category(et, vt, tt, member_axis=mx, threshold_axis=ta, want=want, fair=fair, ref_prob=ref_prob)


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
    mx = axis_of(ens, 'member', member_axis, **_MEMBER)
    _check_ensemble(ens, None, mx, 1)
    thr, ta, Q, tname, tcoord = _threshold_operand(ens, thresholds, mx, threshold_axis)
    f = _category_fields(ens, None, thr, mx, ta, ('prob',))['prob']
    return label(ens, f, 'ensemble_probability', drop=(mx,), lead=[(tname, tcoord)], lat=True)


def brier_score(ens, valid, thresholds, member_axis=0, threshold_axis=0):
    """
    The Brier score of every element and threshold, (k_j / M - 1{y <= t_j})^2 with k_j the members at or below t_j; operands
    as in `ensemble_probability`, `valid` as in `ensemble_crps` (a continuous series with one axis fewer raises
    NotImplementedError).  Returns the (Q, ...) field; NaN where a member, the verification or the threshold is missing.
    """
    mx = axis_of(ens, 'member', member_axis, **_MEMBER)
    _check_ensemble(ens, valid, mx, 1)
    thr, ta, Q, tname, tcoord = _threshold_operand(ens, thresholds, mx, threshold_axis)
    f = _category_fields(ens, valid, thr, mx, ta, ('brier',))['brier']
    return label(ens, f, 'brier_score', drop=(mx,), lead=[(tname, tcoord)], lat=True)


def ranked_probability_score(ens, valid, thresholds, fair=False, member_axis=0, threshold_axis=0):
    """
    The ranked probability score of every element: the sum of the Brier scores over the Q thresholds (the Q + 1 categories they
    bound).  fair=True subtracts sum_j k_j (M - k_j) / (M^2 (M - 1)): the score an ensemble of infinitely many members drawn
    like these would get in expectation (needs 2 members).  Operands as in `brier_score`; returns the (...) field.
    """
    mx = axis_of(ens, 'member', member_axis, **_MEMBER)
    _check_ensemble(ens, valid, mx, 2 if fair else 1)
    thr, ta, _, _, _ = _threshold_operand(ens, thresholds, mx, threshold_axis)
    f = _category_fields(ens, valid, thr, mx, ta, ('rps',), fair=fair)['rps']
    return label(ens, f, 'ranked_probability_score', drop=(mx,), lat=True)


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
    mx = axis_of(ens, 'member', member_axis, **_MEMBER)
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
    mx = axis_of(ens, 'member', member_axis, **_MEMBER)
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
    tail = [('threshold', tcoord), ('members_below', np.arange(M + 1)), ('observed', np.arange(2))]
    return label(ens, counts, 'reliability_counts', drop=_without_member(mx, ax), tail=tail, lat=True)
