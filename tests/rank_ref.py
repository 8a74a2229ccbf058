"""
The definition of dlwpcs_time_rank (include/dlwpcs.h) as plain loops, and the case tables of the rank tests.

`reference` walks every row and every pair of rows of every column in Python: it is the definition and serves the small cases.
`reference_rows` keeps the loop over the rows and takes the partners of a row (and the columns) as one numpy comparison; the
tests of this file's own checks (test_rank_ref.py) hold it equal to the loops, and the GPU tests use it where the loops would
take minutes.  `small_alphabet_stats` counts the trend form's pairs of a column whose values come from a few integers by running
sums per value, O(T) per value: the reference of the longest series.

Arrays are (T, E): rows (times) by columns.  b: None (trend form), (T, E) (pair form) or (T,) (index form).
"""
import numpy as np

TREND, PAIR, INDEX = 0, 1, 2
SKIP, PROPAGATE = 0, 1
MODES = (SKIP, PROPAGATE)
MODE_NAMES = {SKIP: 'skip', PROPAGATE: 'propagate'}
FORM_NAMES = {TREND: 'trend', PAIR: 'pair', INDEX: 'index'}
N_STATS = 8
QNAN = np.uint32(0x7fc00000)


def _partner(a, b):
    a = np.asarray(a, dtype=np.float32)
    T, E = a.shape
    if b is None:
        return a, None
    b = np.asarray(b, dtype=np.float32)
    return a, (np.broadcast_to(b[:, None], (T, E)) if b.ndim == 1 else b)


def _midrank(lt, eq):
    return np.float32(lt) + np.float32(0.5) * np.float32(eq + 1)


def reference(a, b=None, mode=SKIP):
    """(rank_a, rank_b or None, stats (8, E) int64) by loops over rows and pairs"""
    a, bb = _partner(a, b)
    T, E = a.shape
    ra = np.full((T, E), np.nan, dtype=np.float32)
    rb = None if bb is None else np.full((T, E), np.nan, dtype=np.float32)
    st = np.zeros((N_STATS, E), dtype=np.int64)
    for e in range(E):
        x = [float(v) for v in a[:, e]]
        y = [float(t) for t in range(T)] if bb is None else [float(v) for v in bb[:, e]]
        P = [t for t in range(T) if x[t] == x[t] and y[t] == y[t]]
        spoiled = mode == PROPAGATE and len(P) < T
        st[0, e] = len(P)
        for t in P:
            lt_a = sum(1 for s in P if x[s] < x[t])
            eq_a = sum(1 for s in P if x[s] == x[t])
            lt_b = sum(1 for s in P if y[s] < y[t])
            eq_b = sum(1 for s in P if y[s] == y[t])
            if not spoiled:
                ra[t, e] = _midrank(lt_a, eq_a)
                if rb is not None:
                    rb[t, e] = _midrank(lt_b, eq_b)
            st[6, e] += (eq_a - 1) * (2 * eq_a + 5)
            st[7, e] += (eq_b - 1) * (2 * eq_b + 5)
        for n, i in enumerate(P):
            for j in P[n + 1:]:
                sa = (x[j] > x[i]) - (x[j] < x[i])
                sb = (y[j] > y[i]) - (y[j] < y[i])
                k = 1 if sa * sb > 0 else 2 if sa * sb < 0 else 3 if sa == 0 and sb != 0 else 4 if sb == 0 and sa != 0 else 5
                st[k, e] += 1
        if spoiled:
            st[1:, e] = -1
    return ra, rb, st


def reference_rows(a, b=None, mode=SKIP):
    """`reference` with the partners of a row, and the columns, taken together"""
    a, bb = _partner(a, b)
    T, E = a.shape
    present = ~np.isnan(a) if bb is None else ~np.isnan(a) & ~np.isnan(bb)
    y = np.broadcast_to(np.arange(T, dtype=np.float32)[:, None], (T, E)) if bb is None else bb
    lt = np.zeros((2, T, E), dtype=np.int64)
    eq = np.zeros((2, T, E), dtype=np.int64)
    st = np.zeros((N_STATS, E), dtype=np.int64)
    st[0] = present.sum(axis=0)
    with np.errstate(invalid='ignore'):
        for i in range(T):
            for k, v in enumerate((a, y)):
                lt[k, i] = (present & (v < v[i])).sum(axis=0)
                eq[k, i] = (present & (v == v[i])).sum(axis=0)
            ok = present[i + 1:] & present[i]
            sa = np.sign((a[i + 1:] > a[i]).astype(np.int8) - (a[i + 1:] < a[i]).astype(np.int8))
            sb = np.sign((y[i + 1:] > y[i]).astype(np.int8) - (y[i + 1:] < y[i]).astype(np.int8))
            pr = sa * sb
            st[1] += (ok & (pr > 0)).sum(axis=0)
            st[2] += (ok & (pr < 0)).sum(axis=0)
            st[3] += (ok & (sa == 0) & (sb != 0)).sum(axis=0)
            st[4] += (ok & (sb == 0) & (sa != 0)).sum(axis=0)
            st[5] += (ok & (sa == 0) & (sb == 0)).sum(axis=0)
    for k in range(2):
        st[6 + k] = np.where(present, (eq[k] - 1) * (2 * eq[k] + 5), 0).sum(axis=0)
    spoiled = (st[0] < T) if mode == PROPAGATE else np.zeros(E, dtype=bool)
    st[1:, spoiled] = -1
    out = []
    for k in range(2):
        r = lt[k].astype(np.float32) + np.float32(0.5) * (eq[k] + 1).astype(np.float32)
        out.append(np.where(present & ~spoiled[None, :], r, np.float32(np.nan)).astype(np.float32))
    return out[0], (None if bb is None else out[1]), st


def small_alphabet_stats(a):
    """the trend form's statistics of (T, E) columns without NaN whose values are a few distinct numbers: per value the running
    count of earlier rows with a smaller, a larger and the same value"""
    a = np.asarray(a, dtype=np.float32)
    T, E = a.shape
    assert not np.isnan(a).any()
    vals = np.unique(a)
    assert len(vals) <= 16
    before = {v: np.cumsum(a == v, axis=0, dtype=np.int64) - (a == v) for v in vals}      # rows before t that hold v
    st = np.zeros((N_STATS, E), dtype=np.int64)
    st[0] = T
    for v in vals:
        at = a == v
        for w in vals:
            k = 1 if w < v else 2 if w > v else 3
            st[k] += np.where(at, before[w], 0).sum(axis=0)
        g = at.sum(axis=0).astype(np.int64)
        st[6] += g * (g - 1) * (2 * g + 5)
    return st


def tie3_by_groups(column):
    """sum of g (g - 1) (2 g + 5) over the groups of equal values of the present entries of one column"""
    groups = {}
    for v in column:
        if v == v:
            groups[float(v) + 0.0] = groups.get(float(v) + 0.0, 0) + 1        # (-0.0 + 0.0 = +0.0: one group)
    return sum(g * (g - 1) * (2 * g + 5) for g in groups.values())


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ---- data -------------------------------------------------------------------------------------------------------------------
VALUES = ('noise', 'ties', 'special', 'equal', 'rising', 'falling')
HOLES = ('none', 'scattered', 'column', 'b only')


def make(rng, T, E, form, values='noise', holes='none'):
    """(a, b): float32 (T, E) and None / (T, E) / (T,)"""
    def field(shape):
        if values == 'ties':
            return rng.integers(0, 3, shape).astype(np.float32)
        x = rng.standard_normal(shape).astype(np.float32)
        if values == 'special':
            pick = rng.random(shape)
            x = np.where(pick < 0.1, np.float32(np.inf), x)
            x = np.where((pick >= 0.1) & (pick < 0.2), np.float32(-np.inf), x)
            x = np.where((pick >= 0.2) & (pick < 0.3), np.float32(0.0), x)
            x = np.where((pick >= 0.3) & (pick < 0.4), np.float32(-0.0), x)
        return x.astype(np.float32)
    a = field((T, E))
    t = np.arange(T, dtype=np.float32)
    if values == 'equal':
        a[:, 0] = 2.5
    if values == 'rising':
        a[:, 0] = t
    if values == 'falling':
        a[:, 0] = -t
    b = None if form == TREND else field((T, E)) if form == PAIR else field((T,))
    if values in ('equal', 'rising', 'falling') and form == PAIR:
        b[:, 0] = a[:, 0]
    if holes == 'scattered':
        a[rng.random((T, E)) < 0.08] = np.nan
        if b is not None:
            b[rng.random(b.shape) < 0.08] = np.nan
    if holes == 'column':
        a[:, E // 2] = np.nan
        if T > 2:
            a[T // 2, -1] = np.nan
    if holes == 'b only' and b is not None:
        b[rng.random(b.shape) < 0.1] = np.nan
    return a, b


def size_cases():
    """rows around a block of 8, a super-block of 32, a wave; columns around a chunk, a wave and a tile edge; all forms, modes,
    value kinds and hole kinds met at least once"""
    rows = (1, 2, 3, 31, 32, 33, 63, 64, 65)
    cols = (3, 4, 5, 63, 64, 65, 8, 130, 12)
    out = []
    for i, T in enumerate(rows):
        form = (TREND, PAIR, INDEX)[i % 3]
        out.append(dict(T=T, E=cols[i], form=form, mode=MODES[i % 2], values=VALUES[i % len(VALUES)], holes=HOLES[i % len(HOLES)]))
    # every form x mode x hole kind at one size off the block and tile grid
    for form in (TREND, PAIR, INDEX):
        for mode in MODES:
            for holes in HOLES:
                out.append(dict(T=45, E=70, form=form, mode=mode, values='ties' if holes == 'none' else 'special', holes=holes))
    for values in VALUES:
        out.append(dict(T=37, E=9, form=PAIR, mode=SKIP, values=values, holes='none'))
        out.append(dict(T=37, E=9, form=TREND, mode=SKIP, values=values, holes='none'))
    return out


def case_id(c):
    return 'T%d-E%d-%s-%s-%s-%s' % (c['T'], c['E'], FORM_NAMES[c['form']], MODE_NAMES[c['mode']], c['values'], c['holes'].replace(' ', '_'))
