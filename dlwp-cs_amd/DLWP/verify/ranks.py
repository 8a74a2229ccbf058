"""
Rank statistics along time, per grid point: `time_ranks` gives every time its mid-rank among the times of its grid point (the start
of probability-integral and normal-score transforms and of rank-based composites), `kendall_tau` the rank correlation tau-b of
two series with its tie-corrected test, `mann_kendall` the distribution-free trend test that belongs beside the slope of
`time_regression`, `spearman_correlation` the Pearson correlation of the ranks.  They are the tools for skewed variables, where a
moment correlation is the story of a handful of events.

All rest on counts over the pairs of times of a column.  Values on a HIP device are counted there by dlwpcs_time_rank
(include/dlwpcs.h states the definition) and ranks stay there; numpy values take the host twin `_rank_host`, which yields the same
integers and the same mid-ranks by another route.  Neither falls back to the other.  Everything above the integers -- tau, the
variance of S, z and p -- is the same float64 host code for both, on the eight counts per grid point (those are downloaded), so
the two paths give equal records, not merely close ones.  Sen's slope (the median of the pairwise slopes) is not provided.
"""
import math

import numpy as np

from ..labelled import axis_of, device_scope, host as _host, is_tensor as _is_tensor, label, on_device as _on_device, raw as _raw
from .scores import _dev_operand
from .timeseries import lag_correlation

_STATS = ('n_valid', 'concordant', 'discordant', 'tie_a', 'tie_b', 'tie_both', 'tie3_a', 'tie3_b')
_erfc = np.vectorize(math.erfc, otypes=[np.float64])


class KendallTau(object):
    """
    What `kendall_tau` returns, every field labelled like the first input without the time dim: float64 `tau` (tau-b), `S` =
    concordant - discordant, `var_S` (the normal approximation with all three tie terms), `z` (continuity-corrected), `p`
    (two-sided), and int64 `n` (times present in both series).  NaN where fewer than two times are present, where a series is
    constant (tau, z, p) and where missing='propagate' met a missing time.  `counts`: the eight integers of the kernel, a leading
    axis in the order of DLWP.ops.RANK_STATISTICS.
    """
    __slots__ = ('tau', 'S', 'var_S', 'z', 'p', 'n', 'counts', 'missing')

    def __init__(self, fields, counts, missing):
        for k in ('tau', 'S', 'var_S', 'z', 'p', 'n'):
            setattr(self, k, fields[k])
        self.counts, self.missing = counts, missing

    def __repr__(self):
        return "%s(missing='%s')" % (type(self).__name__, self.missing)


class MannKendall(KendallTau):
    """What `mann_kendall` returns: the fields of `KendallTau` for a series against time (S > 0: rising)."""
    __slots__ = ()


def _rank_host(a, b=None, axis=0, missing='skip', ranks=True, stats=True):
    """
    The definition of dlwpcs_time_rank restated with vectorised numpy: (rank_a, rank_b, stats), float32 mid-ranks of a's shape
    (rank_b: None without a b) and int64 stats with a leading axis of the eight counts and `axis` one long; None for what was not
    asked.  Values are compared as float32.  b: None (against time), an array of a's shape or a vector of its rows.  The ranks
    come from a sort and the runs of equal neighbours, the pair counts from one vector comparison per distance between rows.
    """
    va = np.moveaxis(np.asarray(a, dtype=np.float32), axis, 0)
    T, cols = va.shape[0], va.shape[1:]
    E = int(np.prod(cols, dtype=np.int64))
    va = va.reshape(T, E)
    if b is None:
        vb = None
        present = ~np.isnan(va)
    else:
        vb = np.asarray(b, dtype=np.float32)
        if vb.shape == np.shape(a):
            vb = np.moveaxis(vb, axis, 0).reshape(T, E)
        elif vb.shape == (T,):
            vb = np.broadcast_to(vb[:, None], (T, E))
        else:
            raise ValueError('_rank_host: b %s against a %s' % (vb.shape, np.shape(a)))
        present = ~np.isnan(va) & ~np.isnan(vb)
    n = present.sum(axis=0).astype(np.int64)
    spoiled = (n < T) if missing == 'propagate' else np.zeros(E, dtype=bool)
    rows = np.arange(T, dtype=np.int64)[:, None]

    def counts(v):
        """(lt, eq) int64 per entry over the present rows of its column; 0 where absent"""
        key = np.where(present, v, np.float32(np.nan))
        order = np.argsort(key, axis=0, kind='stable')                    # NaN last
        s = np.take_along_axis(key, order, axis=0)
        new = np.ones((T, E), dtype=bool)
        with np.errstate(invalid='ignore'):
            new[1:] = s[1:] != s[:-1]                                        # (-0 == +0: one group)
        first = np.maximum.accumulate(np.where(new, rows, 0), axis=0)      # where the run of equals begins
        nxt = np.where(new, rows, T)
        nxt = np.concatenate([nxt[1:], np.full((1, E), T, dtype=np.int64)], axis=0)
        end = np.minimum.accumulate(nxt[::-1], axis=0)[::-1]               # where the next run begins
        end = np.minimum(end, n[None, :])
        lt = np.zeros((T, E), dtype=np.int64)
        eq = np.zeros((T, E), dtype=np.int64)
        np.put_along_axis(lt, order, first, axis=0)
        np.put_along_axis(eq, order, end - first, axis=0)
        return np.where(present, lt, 0), np.where(present, eq, 0)

    def midrank(lt, eq):
        r = lt.astype(np.float32) + np.float32(0.5) * (eq + 1).astype(np.float32)
        r = np.where(present & ~spoiled[None, :], r, np.float32(np.nan)).astype(np.float32)
        return np.moveaxis(r.reshape((T,) + cols), 0, axis)

    zero = np.zeros((T, E), dtype=np.int64)
    lta, eqa = counts(va) if T else (zero, zero)
    ltb, eqb = counts(vb) if T and vb is not None else (zero, zero)
    ra = midrank(lta, eqa) if ranks else None
    rb = midrank(ltb, eqb) if ranks and vb is not None else None
    st = None
    if stats:
        st = np.zeros((8, E), dtype=np.int64)
        st[0] = n
        xa = np.where(present, va, np.float32(np.nan))
        xb = None if vb is None else np.where(present, vb, np.float32(np.nan))
        with np.errstate(invalid='ignore'):
            for d in range(1, T):
                a0, a1 = xa[:-d], xa[d:]
                la, ga, ea = a0 < a1, a0 > a1, a0 == a1
                if xb is None:
                    st[1] += la.sum(axis=0)
                    st[2] += ga.sum(axis=0)
                    st[3] += ea.sum(axis=0)
                else:
                    b0, b1 = xb[:-d], xb[d:]
                    lb, gb, eb = b0 < b1, b0 > b1, b0 == b1
                    st[1] += ((la & lb) | (ga & gb)).sum(axis=0)
                    st[2] += ((la & gb) | (ga & lb)).sum(axis=0)
                    st[3] += (ea & ~eb).sum(axis=0)
                    st[4] += (eb & ~ea).sum(axis=0)
                    st[5] += (ea & eb).sum(axis=0)
        st[6] = np.where(present, (eqa - 1) * (2 * eqa + 5), 0).sum(axis=0)
        if xb is not None:
            st[7] = np.where(present, (eqb - 1) * (2 * eqb + 5), 0).sum(axis=0)
        st[1:, spoiled] = -1
        st = np.moveaxis(st.reshape((8, 1) + cols), 1, axis + 1)
    return ra, rb, st


def _form(a, b, ax, name):
    if b is None:
        return 'trend'
    sa, sb = tuple(int(s) for s in _raw(a).shape), tuple(int(s) for s in _raw(b).shape)
    if sa == sb:
        return 'pair'
    if len(sb) == 1 and sb[0] == sa[ax]:
        return 'index'
    raise ValueError('%s: the second series %s must have the shape of the first %s or be a vector of its %d times' % (name, sb, sa, sa[ax]))


def _run(a, b, axis, missing, name, ranks=False, stats=False):
    """(time axis, rank_a, rank_b, stats): device tensors where an input lies on a device, else numpy; stats without the time
    axis, (8, ...)"""
    if missing not in ('skip', 'propagate'):
        raise ValueError("%s: 'missing' must be 'skip' or 'propagate'" % name)
    if len(_raw(a).shape) < 1:
        raise ValueError('%s: the series has no time axis' % name)
    ax = axis_of(a, 'time', explicit=axis)
    form = _form(a, b, ax, name)
    if _on_device(a, b):
        import torch
        from .. import ops as dops
        for v in (_raw(a), None if b is None else _raw(b)):
            if _is_tensor(v) and v.is_cuda and v.dtype != torch.float32:
                raise TypeError('%s: device values must be float32, got %s' % (name, v.dtype))
        with device_scope(a, b) as dev:
            at = _dev_operand(a, dev)
            bt = None if b is None else _dev_operand(b, dev)
            res = dops.time_rank(at, bt, row_axis=ax, missing=missing, ranks=ranks, stats=stats)
            res = list(res) if isinstance(res, tuple) else [res]
            ra = res.pop(0) if ranks else None
            rb = res.pop(0) if ranks and form != 'trend' else None
            st = res.pop(0).squeeze(ax + 1) if stats else None
            return ax, ra, rb, st
    ha = np.asarray(_host(a))
    hb = None if b is None else np.asarray(_host(b))
    ra, rb, st = _rank_host(ha, hb, ax, missing, ranks, stats)
    return ax, ra, rb, (None if st is None else np.squeeze(st, axis=ax + 1))


def time_ranks(x, pct=False, axis=None, missing='skip'):
    """
    The mid-rank of every time among the times of its grid point: 1 + the number of smaller values + half the number of other
    equal ones, float32, labelled like x; NaN where the value is missing (missing='propagate': at every time of a grid point
    with a missing one).  Device values are ranked there (dlwpcs_time_rank) and the result stays there.

    :param pct: divide by n_valid + 1: the plotting positions in (0, 1) that a normal-score transform starts from
    :param axis: the time axis, a position or a dim name; None: the 'time' dim of a labelled input, else axis 0
    """
    ax, r, _, st = _run(x, None, axis, missing, 'time_ranks', ranks=True, stats=bool(pct))
    if pct:
        if _is_tensor(r):
            import torch
            r = r / (st[0] + 1).to(torch.float32).unsqueeze(ax)
        else:
            r = (r / np.expand_dims((st[0] + 1).astype(np.float32), ax)).astype(np.float32)
    return label(x, r, 'time_ranks')


def _test(st):
    """the float64 fields from the (8, ...) int64 counts on the host"""
    n, C, D, Ta, Tb, Tab, t3a, t3b = (st[k].astype(np.float64) for k in range(8))
    bad = st[1] < 0                                                       # propagate met a missing time
    with np.errstate(all='ignore'):
        S = C - D
        A2, B2 = 2. * (Ta + Tab), 2. * (Tb + Tab)                         # the sums of g(g-1) over the tie groups
        A3, B3 = (t3a - 9. * A2) / 2., (t3b - 9. * B2) / 2.               # ... of g(g-1)(g-2)
        var = (n * (n - 1.) * (2. * n + 5.) - t3a - t3b) / 18. + A2 * B2 / (2. * n * (n - 1.)) + \
            np.where(n > 2, A3 * B3 / (9. * n * (n - 1.) * (n - 2.)), 0.)
        tau = S / np.sqrt((C + D + Ta) * (C + D + Tb))
        z = np.where(var > 0, (S - np.sign(S)) / np.sqrt(var), np.nan)
        p = np.where(np.isnan(z), np.nan, _erfc(np.abs(np.where(np.isnan(z), 0., z)) / math.sqrt(2.)))
        few = bad | (n < 2)
        S, var, tau, z, p = (np.where(few, np.nan, v) for v in (S, var, tau, z, p))
    return dict(tau=tau, S=S, var_S=var, z=z, p=p, n=st[0].copy())


def _record(cls, x, st, ax, missing, name):
    st = st.cpu().numpy() if _is_tensor(st) else st
    f = _test(st)
    return cls({k: label(x, v, name + '_' + k, drop=(ax,)) for k, v in f.items()}, st, missing)


def kendall_tau(a, b, axis=None, missing='skip'):
    """
    Kendall's tau-b between two series along time, per grid point, with its test: tau = (C - D) / sqrt((C + D + T_a)(C + D + T_b))
    over the concordant, discordant and singly tied pairs of the times present in both; S = C - D with the tie-corrected variance
    of its normal approximation, z = (S - sgn S) / sqrt(var S) and the two-sided p = erfc(|z| / sqrt 2).

    :param a: a `Forecast` (or anything with `.dims`, `.coords`, `.values`), a numpy array or a torch tensor.  float32 values on a
        HIP device are counted there (dlwpcs_time_rank) and only the eight counts per grid point come back; numpy values take
        the host twin, compared as float32
    :param b: a series of a's shape, or a vector of T values shared by every grid point (an index)
    :param axis: the time axis, a position or a dim name; None: the 'time' dim of a labelled input, else axis 0
    :param missing: a time with NaN in either series is missing.  'skip': it is left out; 'propagate': a grid point with any
        missing time gets NaN
    :return: a `KendallTau`
    """
    if b is None:
        raise ValueError('kendall_tau: a second series is needed (mann_kendall tests a series against time)')
    ax, _, _, st = _run(a, b, axis, missing, 'kendall_tau', stats=True)
    return _record(KendallTau, a, st, ax, missing, 'kendall')


def mann_kendall(x, axis=None, missing='skip'):
    """
    The Mann-Kendall trend test along time, per grid point: S = the sum over the pairs of times i < j of sgn(x_j - x_i), its
    variance corrected for ties, z with the continuity correction, the two-sided p and tau = S over the pairs that are not tied:
    the significance map to put beside the slope of `time_regression`.  Arguments as for `kendall_tau`.

    :return: a `MannKendall`
    """
    ax, _, _, st = _run(x, None, axis, missing, 'mann_kendall', stats=True)
    return _record(MannKendall, x, st, ax, missing, 'mann_kendall')


def spearman_correlation(a, b, axis=None, missing='skip'):
    """
    Spearman's rank correlation along time, per grid point: both series are ranked over the times present in both (mid-ranks), and
    the ranks are correlated by `lag_correlation` at lag 0 (on the device: dlwpcs_time_lag, float32; on the host float64).  b: a
    series of a's shape or a vector of T values.  Labelled like a without the time dim.
    """
    if b is None:
        raise ValueError('spearman_correlation: a second series is needed')
    ax, ra, rb, _ = _run(a, b, axis, missing, 'spearman_correlation', ranks=True)
    r = _raw(lag_correlation(ra, rb, lags=[0], axis=ax))
    r = r.squeeze(ax) if _is_tensor(r) else np.squeeze(r, axis=ax)
    return label(a, r, 'spearman_correlation', drop=(ax,))
