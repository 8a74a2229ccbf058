"""
Spells along time: the maximal runs of times on which a condition `x op threshold` holds, per grid point.  `spell_statistics`
counts them (heat-wave days above a climatological quantile, blocked spells of at least five days, the longest run below a
threshold), `spell_length` and `spell_position` give every time the length of its spell and its place inside it, `spell_mask` the
0 / 1 / NaN mask of the times inside a qualifying spell, which `group_mean` turns into seasonal frequencies and
`bootstrap_interval` into intervals.

Values on a HIP device go through dlwpcs_time_spell (include/dlwpcs.h states the definition) and every result stays there;
numpy values take the host twin `_spell_host`, the same comparisons in float32 and the same integers.  Neither falls back to
the other.
"""
import numpy as np

from ..labelled import axis_of, device_scope, host as _host, is_tensor as _is_tensor, label, on_device as _on_device, raw as _raw
from .scores import _dev_operand
from .climatology import ClimatologyLookup

_OPS = ('>', '>=', '<', '<=')
_FIELDS = ('count', 'rows', 'longest', 'longest_start', 'n_valid', 'n_true', 'frequency', 'mean_length')


class SpellStatistics(object):
    """
    What `spell_statistics` returns, every field labelled like the input without the time dim: int32 `count` (qualifying spells),
    `rows` (the sum of their lengths), `longest` (0 if none), `longest_start` (the position along time where the first spell of
    that length begins, -1 if none), `n_valid` (times that are not missing), `n_true` (times on which the condition holds,
    whatever min_length); float64 `frequency` = rows / n_valid and `mean_length` = rows / count, NaN on 0 / 0 and where
    missing='propagate' met a missing time (the int fields but n_valid are -1 there).  `op`, `min_length`, `missing`: what was used.
    """
    __slots__ = _FIELDS + ('op', 'min_length', 'missing')

    def __init__(self, fields, op, min_length, missing):
        for k in _FIELDS:
            setattr(self, k, fields[k])
        self.op, self.min_length, self.missing = op, int(min_length), missing

    def __repr__(self):
        return "SpellStatistics(op='%s', min_length=%d, missing='%s')" % (self.op, self.min_length, self.missing)


def _compare(x, h, op):
    with np.errstate(invalid='ignore'):
        return x > h if op == '>' else (x >= h if op == '>=' else (x < h if op == '<' else x <= h))


def _spell_host(x, table, index=None, op='>', min_length=1, axis=0, missing='break'):
    """
    The definition of dlwpcs_time_spell restated with numpy: (pos, len, stats) int32, pos and len of x's shape, stats with a
    leading axis of the six statistics and `axis` one long.  x and the threshold are compared as float32.  table broadcasts
    against x with K rows on `axis`; index (T ints) names the table row of every time, None: row 0.
    """
    v = np.moveaxis(np.asarray(x, dtype=np.float32), axis, 0)
    tb = np.asarray(table, dtype=np.float32)
    tb = tb.reshape((1,) * (v.ndim - tb.ndim) + tb.shape) if tb.ndim < v.ndim else tb
    tb = np.moveaxis(tb, axis, 0)
    T = v.shape[0]
    h = tb[np.asarray(index, dtype=np.int64)] if index is not None else tb[:1]
    c = np.broadcast_to(_compare(v, h, op), v.shape)
    m = np.broadcast_to(np.isnan(v) | np.isnan(h), v.shape)
    t = np.arange(T, dtype=np.int64).reshape((T,) + (1,) * (v.ndim - 1))
    if T:
        before = np.maximum.accumulate(np.where(c, -1, t), axis=0)                     # the last false row at or before t
        after = np.minimum.accumulate(np.where(c, T, t)[::-1], axis=0)[::-1]           # the first false row at or behind t
    else:
        before = after = np.zeros(v.shape, dtype=np.int64)
    n = after - before - 1
    q = c & (n >= int(min_length))
    pos = np.where(q, t - before, 0).astype(np.int32)
    ln = np.where(q, n, 0).astype(np.int32)
    stats = np.zeros((6, 1) + v.shape[1:], dtype=np.int32)
    stats[0, 0] = (~m).sum(axis=0)
    stats[1, 0] = c.sum(axis=0)
    stats[2, 0] = (q & (pos == 1)).sum(axis=0)
    stats[3, 0] = q.sum(axis=0)
    if T:
        stats[4, 0] = ln.max(axis=0)
        stats[5, 0] = np.where(stats[4, 0] > 0, ln.argmax(axis=0), -1)                # (argmax: the first row of the first longest)
    else:
        stats[5, 0] = -1
    if missing == 'propagate':
        bad = m.any(axis=0)
        pos = np.where(bad, np.int32(-1), pos)
        ln = np.where(bad, np.int32(-1), ln)
        stats[1:, 0] = np.where(bad, np.int32(-1), stats[1:, 0])
    return np.moveaxis(pos, 0, axis), np.moveaxis(ln, 0, axis), np.moveaxis(stats, 1, axis + 1)


def _align(threshold, x, ax, name):
    """the threshold array shaped to x's number of dims with the time axis one long: by dim names where both carry them, else by
    numpy's trailing-axis rule"""
    h = _raw(threshold)
    nd = len(_raw(x).shape)
    hs = tuple(int(s) for s in h.shape)
    if hasattr(threshold, 'dims') and hasattr(x, 'dims'):
        xd, td = tuple(x.dims), tuple(threshold.dims)
        if [d for d in td if d not in xd] or [d for d in xd if d in td] != list(td):
            raise ValueError('%s: the threshold dims %s are not those of the data %s in their order' % (name, td, xd))
        shape = tuple(hs[td.index(d)] if d in td else 1 for d in xd)
    else:
        if len(hs) > nd:
            raise ValueError('%s: threshold %s has more dims than the data %s' % (name, hs, tuple(_raw(x).shape)))
        shape = (1,) * (nd - len(hs)) + hs
    if shape[ax] != 1:
        raise ValueError('%s: an array threshold has the time axis one long or not at all, got %s (a table needs its rows)' % (name, hs))
    for a, (e, xe) in enumerate(zip(shape, _raw(x).shape)):
        if e != 1 and e != int(xe):
            raise ValueError('%s: threshold %s does not broadcast against the data %s' % (name, hs, tuple(_raw(x).shape)))
    return h.reshape(shape)


def _jobs(x, threshold, ax, name):
    """[(lead or None, time axis of that part, table, rows or None)]: what each kernel call compares against.  lead: the index on
    axis 0 of x that the part is."""
    shape = tuple(int(s) for s in _raw(x).shape)
    T = shape[ax]
    if isinstance(threshold, (bool, np.bool_)):
        raise TypeError('%s: the threshold must be a number, an array, a ClimatologyLookup or a (table, rows) pair' % name)
    if isinstance(threshold, (int, float, np.integer, np.floating)):
        return [(None, ax, float(threshold), None)]
    if isinstance(threshold, ClimatologyLookup):
        table, rows, tax = threshold.table, threshold.rows, threshold.row_axis
    elif isinstance(threshold, tuple):
        if len(threshold) != 2:
            raise ValueError('%s: a tuple threshold is (table, rows)' % name)
        table, rows = threshold
        rows = np.asarray(rows)
        if rows.size and rows.dtype.kind not in 'iu':
            raise ValueError('%s: the rows of a (table, rows) threshold must be ints, got %s' % (name, rows.dtype))
        tax = None
    else:
        if not (hasattr(_raw(threshold), 'shape')):
            raise TypeError('%s: the threshold must be a number, an array, a ClimatologyLookup or a (table, rows) pair' % name)
        return [(None, ax, _align(threshold, x, ax, name), None)]
    tb = _raw(table)
    ts = tuple(int(s) for s in tb.shape)
    if rows.ndim == 1:
        lead, want, axp = False, shape, ax
    elif rows.ndim == 2:
        if ax == 0 or rows.shape[0] != shape[0]:
            raise ValueError('%s: a row table over %d forecast hours needs them on axis 0 of the data %s, in front of time' %
                             (name, rows.shape[0], shape))
        lead, want, axp = True, shape[1:], ax - 1
    else:
        raise ValueError('%s: the row table must be (time,) or (f_hour, time), got %s' % (name, rows.shape))
    if tax is not None and tax != axp:
        raise ValueError('%s: the lookup has its rows on axis %d, the data has time on axis %d' % (name, tax, axp))
    if rows.shape[-1] != T:
        raise ValueError('%s: %d table rows are named for %d times' % (name, rows.shape[-1], T))
    if len(ts) != len(want) or ts[axp] < 1 or any(e != 1 and e != w for a, (e, w) in enumerate(zip(ts, want)) if a != axp):
        raise ValueError('%s: the threshold table %s does not fit the data %s with its rows on axis %d' % (name, ts, want, axp))
    if rows.size and (rows.min() < 0 or rows.max() >= ts[axp]):
        raise IndexError('%s: threshold row out of range of the %d table rows' % (name, ts[axp]))
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    if not lead:
        return [(None, ax, tb, rows)]
    return [(f, axp, tb, rows[f]) for f in range(shape[0])]


def _check(op, min_length, missing, name):
    if op not in _OPS:
        raise ValueError("%s: op must be '>', '>=', '<' or '<=', got %r" % (name, op))
    if isinstance(min_length, bool) or not isinstance(min_length, (int, np.integer)) or int(min_length) < 1:
        raise ValueError('%s: min_length must be an int of at least 1, got %r' % (name, min_length))
    if missing not in ('break', 'propagate'):
        raise ValueError("%s: 'missing' must be 'break' or 'propagate'" % name)


def _run(x, threshold, op, min_length, axis, missing, name, position=False, length=False, statistics=False, absent=False):
    """(time axis, [position, length, statistics, absent] with None for what was not asked): device tensors where any input lies on
    a device, else numpy.  statistics: (6, ...) with the time axis dropped.  absent: bool, True where the entry or its threshold
    is NaN."""
    _check(op, min_length, missing, name)
    v = _raw(x)
    if len(v.shape) < 1:
        raise ValueError('%s: the series has no time axis' % name)
    ax = axis_of(x, 'time', explicit=axis)
    jobs = _jobs(x, threshold, ax, name)
    tables = [j[2] for j in jobs[:1] if not isinstance(j[2], float)]
    parts = []
    if _on_device(x, *tables):
        import torch
        from .. import ops as dops
        if _is_tensor(v) and v.is_cuda and v.dtype != torch.float32:
            raise TypeError('%s: device values must be float32, got %s' % (name, v.dtype))
        with device_scope(x, *tables) as dev:
            xv = _dev_operand(x, dev)
            tb = None if not tables else _dev_operand(tables[0], dev)
            for lead, axp, table, rows in jobs:
                part = xv if lead is None else xv[lead]
                th = table if tb is None else tb
                res = dops.time_spell(part, th, rows, op=op, min_length=int(min_length), row_axis=axp, missing=missing,
                                      position=position, length=length, statistics=statistics) if (position or length or statistics) else ()
                res = list(res) if isinstance(res, tuple) else [res]
                out = [res.pop(0) if want else None for want in (position, length, statistics)]
                if out[2] is not None:
                    out[2] = out[2].squeeze(axp + 1)
                if absent:
                    gone = torch.isnan(part)
                    if tb is not None:
                        tn = torch.isnan(tb)
                        if rows is not None:
                            tn = tn.index_select(axp, torch.from_numpy(rows.astype(np.int64)).to(dev))
                        gone = gone | tn
                    elif table != table:
                        gone = torch.ones_like(gone)
                    out.append(gone)
                else:
                    out.append(None)
                parts.append(out)
            stack = lambda k, a: None if parts[0][k] is None else (parts[0][k] if jobs[0][0] is None else       # noqa: E731
                                                                   torch.stack([p[k] for p in parts], dim=a))
            return ax, [stack(0, 0), stack(1, 0), stack(2, 1), stack(3, 0)]
    xv = np.asarray(_host(x))
    for lead, axp, table, rows in jobs:
        part = xv if lead is None else xv[lead]
        th = np.float32(table) if isinstance(table, float) else np.asarray(_host(table), dtype=np.float32)
        pos, ln, st = _spell_host(part, th, rows, op, int(min_length), axp, missing)
        gone = None
        if absent:
            p32 = np.moveaxis(np.asarray(part, dtype=np.float32), axp, 0)
            tn = np.isnan(np.moveaxis(th.reshape((1,) * (p32.ndim - th.ndim) + th.shape), axp, 0))
            tn = tn[rows.astype(np.int64)] if rows is not None else tn
            gone = np.moveaxis(np.isnan(p32) | tn, 0, axp)
        parts.append([pos if position else None, ln if length else None, np.squeeze(st, axis=axp + 1) if statistics else None, gone])
    stack = lambda k, a: None if parts[0][k] is None else (parts[0][k] if jobs[0][0] is None else               # noqa: E731
                                                           np.stack([p[k] for p in parts], axis=a))
    return ax, [stack(0, 0), stack(1, 0), stack(2, 1), stack(3, 0)]


def spell_statistics(x, threshold, op='>', min_length=1, axis=None, missing='break'):
    """
    The statistics of the spells of `x op threshold` along time, per grid point (every dim but time is a column: a
    (f_hour, time, ...) forecast gets them per lead).

    :param x: a `Forecast` (or anything with `.dims`, `.coords`, `.values`), a numpy array or a torch tensor.  float32 values on a
        HIP device are scanned there (dlwpcs_time_spell) and the result stays there; numpy values take the host twin, compared
        as float32
    :param threshold: a number; an array or `Forecast` that broadcasts against x with the time axis one long or absent (a
        labelled one is aligned by dim names); or one table row per time: a `ClimatologyLookup` (`daily_climo_time_series(...,
        lazy=True)` of a `climatology_quantiles` table) or a pair (table, rows) with the table's rows where x has time and rows
        (time,) ints.  Rows of shape (f_hour, time), as a lookup over forecast hours has them, are served one lead at a time
        against x with f_hour on axis 0
    :param op: '>', '>=', '<' or '<='; a comparison with NaN on either side is false and the time counts as missing
    :param min_length: the times a spell needs to qualify (it may exceed the series: nothing qualifies)
    :param axis: the time axis, a position or a dim name; None: the 'time' dim of a labelled input, else axis 0
    :param missing: 'break': a missing time ends a spell like any time off the condition; 'propagate': a grid point with any
        missing time has -1 in every int field but n_valid, and NaN frequency and mean_length
    :return: a `SpellStatistics`
    """
    name = 'spell_statistics'
    ax, (_, _, st, _) = _run(x, threshold, op, min_length, axis, missing, name, statistics=True)
    n_valid, n_true, count, rows, longest, start = (st[k] for k in range(6))
    if _is_tensor(st):
        import torch
        nan = torch.full((), float('nan'), dtype=torch.float64, device=st.device)
        r = rows.to(torch.float64)
        freq = torch.where(rows < 0, nan, r / n_valid.to(torch.float64))
        mean = torch.where(rows < 0, nan, r / count.to(torch.float64))
    else:
        with np.errstate(all='ignore'):
            r = rows.astype(np.float64)
            freq = np.where(rows < 0, np.nan, r / n_valid.astype(np.float64))
            mean = np.where(rows < 0, np.nan, r / count.astype(np.float64))
    vals = dict(count=count, rows=rows, longest=longest, longest_start=start, n_valid=n_valid, n_true=n_true, frequency=freq,
                mean_length=mean)
    return SpellStatistics({k: label(x, v, 'spell_' + k, drop=(ax,)) for k, v in vals.items()}, op, min_length, missing)


def spell_length(x, threshold, op='>', min_length=1, axis=None, missing='break'):
    """Per time and grid point the length of the qualifying spell that holds it, 0 outside one (int32, x's dims; -1 where
    missing='propagate' met a missing time).  The arguments are those of `spell_statistics`."""
    _, (_, ln, _, _) = _run(x, threshold, op, min_length, axis, missing, 'spell_length', length=True)
    return label(x, ln, 'spell_length')


def spell_position(x, threshold, op='>', min_length=1, axis=None, missing='break'):
    """Per time and grid point its 1-based place inside its qualifying spell, 0 outside one (int32, x's dims; -1 where
    missing='propagate' met a missing time).  The arguments are those of `spell_statistics`."""
    _, (pos, _, _, _) = _run(x, threshold, op, min_length, axis, missing, 'spell_position', position=True)
    return label(x, pos, 'spell_position')


def spell_mask(x, threshold, op='>', min_length=1, axis=None, missing='break'):
    """The float32 mask of the times inside a qualifying spell: 1 inside, 0 outside, NaN where the entry (or its threshold) is
    missing, and under missing='propagate' at every time of a grid point with a missing one.  x's dims: `group_mean` over
    seasons gives spell frequencies, `bootstrap_interval` their sampling uncertainty.  The arguments are those of
    `spell_statistics`."""
    _, (_, ln, _, gone) = _run(x, threshold, op, min_length, axis, missing, 'spell_mask', length=True, absent=True)
    if _is_tensor(ln):
        import torch
        mask = (ln > 0).to(torch.float32)
        mask = torch.where(gone | (ln < 0), torch.full((), float('nan'), dtype=torch.float32, device=ln.device), mask)
    else:
        mask = np.where(gone | (ln < 0), np.float32(np.nan), (ln > 0).astype(np.float32)).astype(np.float32)
    return label(x, mask, 'spell_mask')
