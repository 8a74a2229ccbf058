"""
Reference, combine rule, case tables and series makers of the spell tests (test_spell_ref.py, test_spell.py, test_gpu_spell.py,
test_gpu_spell_verify.py).  Not a test module.

reference(): the definition of dlwpcs_time_spell (include/dlwpcs.h) restated with plain loops per column: c = x cmp h as float32
(false with a NaN on either side), m = isnan(x) or isnan(h); a spell is a maximal interval of rows with c true, it qualifies with
at least min_length rows; pos is the 1-based place inside the qualifying spell and len its length, 0 outside; the statistics are
n_valid, n_true, n_spells, spell_rows, longest, longest_start (-1 if none); PROPAGATE puts -1 everywhere but in n_valid in a
column with a missing row.  reference_vector() is the same statement vectorised over columns and rows (run ids by cumulative
sums), for the larger cases.  partial() / join() / finish() restate the slab combine rule.
"""
import itertools

import numpy as np

GT, GE, LT, LE = 0, 1, 2, 3
BREAK, PROPAGATE = 0, 1
OP_NAMES = {GT: '>', GE: '>=', LT: '<', LE: '<='}
MODE_NAMES = {BREAK: 'break', PROPAGATE: 'propagate'}
STATS = ('n_valid', 'n_true', 'n_spells', 'spell_rows', 'longest', 'longest_start')
CLASSES = (1, 2, 4, 8, 16, 32)                      # words of 32 rows a lane holds

ROWS = [1, 2, 31, 32, 33, 64, 65, 100]
COLUMNS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000]     # around a chunk (4), a wave / tile (64) and four tiles
OPS = [GT, GE, LT, LE]
MIN_LENGTHS = ['1', '2', '5', 'T', 'T+1']
PATTERNS = ['red noise', 'all true', 'all false', 'alternating', 'one false', 'word runs', 'exact length', 'tie']
NAN_PATTERNS = ['none', 'one percent', 'nan row', 'nan column', 'one valid', 'nan threshold']
INF_PATTERNS = ['none', 'inf series', 'inf threshold']
THRESHOLDS = ['scalar', 'column', 'variable', 'table']
MODES = [BREAK, PROPAGATE]
TABLE_ROWS = 5                                      # K of the 'table' threshold


def compare(x, h, op):
    x, h = np.float32(x), np.float32(h)
    with np.errstate(invalid='ignore'):
        return [x > h, x >= h, x < h, x <= h][op]


def min_length(T, name):
    return max({'1': 1, '2': 2, '5': 5, 'T': T, 'T+1': T + 1}[name], 1)


def thresholds_of(thr, index, T, E):
    """h[t, e] of a (K, E) or (K, 1) table"""
    idx = np.zeros(T, dtype=np.int64) if index is None else np.asarray(index, dtype=np.int64)
    return np.broadcast_to(np.asarray(thr, dtype=np.float32)[idx], (T, E))


def reference(x, thr, index, op, minlen, mode):
    """x (T, E) float32, thr (K, E) or (K, 1), index (T,) or None -> (pos (T, E), len (T, E), stats (6, E)) int32, plain loops"""
    x = np.asarray(x, dtype=np.float32)
    T, E = x.shape
    thr = np.asarray(thr, dtype=np.float32)
    pos = np.zeros((T, E), dtype=np.int32)
    ln = np.zeros((T, E), dtype=np.int32)
    stats = np.zeros((6, E), dtype=np.int32)
    for e in range(E):
        c, m = [], []
        for t in range(T):
            h = thr[0 if index is None else int(index[t]), e if thr.shape[1] > 1 else 0]
            c.append(bool(compare(x[t, e], h, op)))
            m.append(bool(np.isnan(x[t, e]) or np.isnan(h)))
        n_spells = rows = longest = 0
        start = -1
        t = 0
        while t < T:
            if not c[t]:
                t += 1
                continue
            s = t
            while t < T and c[t]:
                t += 1
            n = t - s
            if n >= minlen:
                n_spells += 1
                rows += n
                if n > longest:
                    longest, start = n, s
                for r in range(s, t):
                    pos[r, e], ln[r, e] = r - s + 1, n
        stats[:, e] = (T - sum(m), sum(c), n_spells, rows, longest, start)
        if mode == PROPAGATE and any(m):
            pos[:, e] = ln[:, e] = -1
            stats[1:, e] = -1
    return pos, ln, stats


def reference_vector(x, thr, index, op, minlen, mode):
    """reference() without loops: a run id per row from the cumulative count of false rows, run lengths by bincount"""
    x = np.asarray(x, dtype=np.float32)
    T, E = x.shape
    h = thresholds_of(thr, index, T, E)
    c = compare(x, h, op)
    m = np.isnan(x) | np.isnan(h)
    stats = np.zeros((6, E), dtype=np.int32)
    stats[0], stats[1] = (~m).sum(0), c.sum(0)
    stats[5] = -1
    pos = np.zeros((T, E), dtype=np.int32)
    ln = np.zeros((T, E), dtype=np.int32)
    if T:
        run = np.cumsum(~c, axis=0) + np.arange(E)[None, :] * (T + 1)         # a run id: the false rows so far, offset per column
        size = np.bincount(run[c], minlength=E * (T + 1))                     # trues of every run
        n = np.where(c, size[run], 0)
        first = np.full(E * (T + 1), T, dtype=np.int64)
        tt = np.broadcast_to(np.arange(T)[:, None], (T, E))
        np.minimum.at(first, run[c], tt[c])
        q = c & (n >= minlen)
        pos = np.where(q, tt - first[run] + 1, 0).astype(np.int32)
        ln = np.where(q, n, 0).astype(np.int32)
        stats[2], stats[3], stats[4] = (pos == 1).sum(0), q.sum(0), ln.max(0)
        stats[5] = np.where(stats[4] > 0, (ln == stats[4][None, :]).argmax(0), -1)
    if mode == PROPAGATE:
        bad = m.any(0)
        pos[:, bad] = -1
        ln[:, bad] = -1
        stats[1:, bad] = -1
    return pos, ln, stats


# ---- the slab combine rule (one column) -------------------------------------------------------------------------------- #

def _close(p, run, start, minlen, tie_earlier=False):
    if run > 0 and run >= minlen:
        p['cnt'] += 1
        p['rows'] += run
        if run > p['longest'] or (tie_earlier and run == p['longest'] and start < p['start']):
            p['longest'], p['start'] = run, start


def partial(c, m, first_row, minlen):
    """the partial of the rows c (bools) that begin at absolute row first_row"""
    n = len(c)
    head = 0
    while head < n and c[head]:
        head += 1
    p = dict(n=n, first=first_row, head=head, tail=head, n_valid=n - int(sum(m)), n_true=int(sum(c)), cnt=0, rows=0, longest=0, start=-1)
    if head == n:
        return p
    tail = 0
    while c[n - 1 - tail]:
        tail += 1
    p['tail'] = tail
    t = head
    while t < n - tail:
        if not c[t]:
            t += 1
            continue
        s = t
        while c[t]:
            t += 1
        _close(p, t - s, first_row + s, minlen)
    return p


def join(a, b, minlen):
    """a before b"""
    assert a['first'] + a['n'] == b['first']
    r = dict(a, n=a['n'] + b['n'], n_valid=a['n_valid'] + b['n_valid'], n_true=a['n_true'] + b['n_true'])
    all_a, all_b = a['head'] == a['n'], b['head'] == b['n']
    if all_a and all_b:
        r['head'] = r['tail'] = r['n']
        return r
    if all_a:
        r['head'], r['tail'] = a['n'] + b['head'], b['tail']
    elif all_b:
        r['tail'] = a['tail'] + b['n']
        return r
    else:
        r['tail'] = b['tail']
        _close(r, a['tail'] + b['head'], b['first'] - a['tail'], minlen)
    r['cnt'] += b['cnt']
    r['rows'] += b['rows']
    if b['longest'] > r['longest']:
        r['longest'], r['start'] = b['longest'], b['start']
    return r


def finish(p, minlen, mode=BREAK):
    """the six statistics of the partial of a whole series"""
    r = dict(p)
    if r['head'] == r['n']:
        _close(r, r['n'], 0, minlen)
    else:
        _close(r, r['head'], 0, minlen, tie_earlier=True)
        _close(r, r['tail'], r['n'] - r['tail'], minlen)
    out = [r['n_valid'], r['n_true'], r['cnt'], r['rows'], r['longest'], r['start']]
    if mode == PROPAGATE and r['n_valid'] < r['n']:
        out[1:] = [-1] * 5
    return out


def cut_sets(T):
    """every way to cut T rows into consecutive pieces: tuples of the first rows of the pieces behind the first"""
    for k in range(T):
        for cuts in itertools.combinations(range(1, T), k):
            yield cuts


# ---- series ------------------------------------------------------------------------------------------------------------ #

def make_case(rng, T, E, pattern, nan_pattern='none', inf_pattern='none', threshold='scalar', minlen=1, n_var=1):
    """(x (T, E) float32, thr (K, E or 1) float32, index (T,) int32 or None).  The patterns are laid against a threshold near 280;
    a 'variable' threshold has one value per block of E / n_var columns and is returned expanded to (K, E)."""
    K = TABLE_ROWS if threshold == 'table' else 1
    if threshold == 'scalar':
        thr = np.full((K, 1), 280., dtype=np.float32)
    elif threshold == 'variable':
        per = (280. + 3. * rng.standard_normal((K, max(n_var, 1)))).astype(np.float32)
        thr = per[:, (np.arange(E) * max(n_var, 1)) // max(E, 1)]
    else:
        thr = (280. + 3. * rng.standard_normal((K, E))).astype(np.float32)
    index = rng.integers(0, K, size=T).astype(np.int32) if threshold == 'table' else None
    if index is not None and T >= K:
        index[rng.permutation(T)[:K]] = np.arange(K)                # every table row is used
    h = thresholds_of(thr, index, T, E).astype(np.float32)
    t = np.arange(T)[:, None]
    if pattern == 'red noise':
        e = rng.standard_normal((T, E))
        for i in range(1, T):
            e[i] = 0.8 * e[i - 1] + 0.6 * e[i]
        up = e > 0
    elif pattern == 'all true':
        up = np.ones((T, E), dtype=bool)
    elif pattern == 'all false':
        up = np.zeros((T, E), dtype=bool)
    elif pattern == 'alternating':
        up = ((t + np.arange(E)[None, :]) % 2).astype(bool)
    elif pattern == 'one false':
        up = np.ones((T, E), dtype=bool)
        up[rng.integers(0, T, size=E), np.arange(E)] = False
    elif pattern == 'word runs':                                   # runs that begin on row 32 k and end on row 32 k - 1
        up = np.broadcast_to(((t // 32 + np.arange(E)[None, :]) % 2).astype(bool), (T, E)).copy()
    elif pattern == 'exact length':                                # a run exactly min_length long, and one a row shorter
        up = np.zeros((T, E), dtype=bool)
        L = min(minlen, T)
        for e in range(E):
            s = int(rng.integers(0, T - L + 1))
            up[s:s + L, e] = True
            s2 = s + L + 1
            if L > 1 and s2 + L - 1 <= T:
                up[s2:s2 + L - 1, e] = True
    elif pattern == 'tie':                                         # two equally long spells: longest_start is the first one's
        up = np.zeros((T, E), dtype=bool)
        L = max(min(minlen, (T - 1) // 2), 1)
        for e in range(E):
            if 2 * L + 1 <= T:
                s = int(rng.integers(0, T - 2 * L))
                up[s:s + L, e] = True
                up[s + L + 1:s + 2 * L + 1, e] = True
            else:
                up[:, e] = True
    else:
        raise ValueError(pattern)
    mag = (0.5 + rng.random((T, E))).astype(np.float32)
    x = (h + np.where(up, mag, -mag)).astype(np.float32)
    if pattern == 'red noise':
        on = rng.random((T, E)) < 0.05                              # some entries exactly on the threshold: > and >= differ
        x = np.where(on, h, x).astype(np.float32)
    if inf_pattern == 'inf series':
        x[rng.random((T, E)) < 0.05] = np.inf
        x[rng.random((T, E)) < 0.05] = -np.inf
    elif inf_pattern == 'inf threshold':
        thr = thr.copy()
        thr[rng.integers(0, K), rng.integers(0, thr.shape[1])] = np.inf
        thr[rng.integers(0, K), rng.integers(0, thr.shape[1])] = -np.inf
    if nan_pattern == 'one percent':
        x[rng.random((T, E)) < 0.01] = np.nan
        x[rng.integers(0, T), rng.integers(0, E)] = np.nan
    elif nan_pattern == 'nan row':
        x[rng.integers(0, T)] = np.nan
    elif nan_pattern == 'nan column':
        x[:, rng.integers(0, E)] = np.nan
    elif nan_pattern == 'one valid':
        r = rng.integers(0, T)
        keep = x[r, :].copy()
        x[:] = np.nan
        x[r] = keep
    elif nan_pattern == 'nan threshold':
        thr = thr.copy()
        thr[rng.integers(0, K), rng.integers(0, thr.shape[1])] = np.nan
    elif nan_pattern != 'none':
        raise ValueError(nan_pattern)
    return x, thr, index


def cases():
    """The size cases of the device test: every (T, columns) of ROWS x COLUMNS, with the operator, min_length, pattern, NaN and inf
    pattern, threshold kind and mode rotating at strides that let each value of each table occur (test_spell_ref.py checks that).
    dict(T, E, op, minlen, minlen_name, pattern, nan, inf, threshold, mode, seed)."""
    out = []
    for it, T in enumerate(ROWS):
        for ie, E in enumerate(COLUMNS):
            i = it * len(COLUMNS) + ie
            mn = MIN_LENGTHS[(i + it) % len(MIN_LENGTHS)]
            out.append(dict(T=T, E=E, op=OPS[i % len(OPS)], minlen=min_length(T, mn), minlen_name=mn,
                            pattern=PATTERNS[(i + i // 8) % len(PATTERNS)], nan=NAN_PATTERNS[(i // 2) % len(NAN_PATTERNS)],
                            inf=INF_PATTERNS[(i // 3) % len(INF_PATTERNS)], threshold=THRESHOLDS[(i + i // 4) % len(THRESHOLDS)],
                            mode=MODES[(i // 5) % len(MODES)], seed=900 + i))
    return out


def case_id(c):
    return 'T%d-E%d-%s-min%s-%s-%s-%s-%s-%s' % (c['T'], c['E'], {GT: 'gt', GE: 'ge', LT: 'lt', LE: 'le'}[c['op']], c['minlen_name'],
                                                 c['pattern'].replace(' ', '_'), c['nan'].replace(' ', '_'), c['inf'].replace(' ', '_'),
                                                 c['threshold'], MODE_NAMES[c['mode']])


def make(c):
    """the series of a case of cases().  The patterns are written for '>': for '<' and '<=' the series is mirrored about its
    threshold, which keeps every run where it is."""
    rng = np.random.default_rng(c['seed'])
    x, thr, index = make_case(rng, c['T'], c['E'], c['pattern'], c['nan'], c['inf'], c['threshold'], c['minlen'],
                              n_var=3 if c['E'] % 3 == 0 else 1)
    if c['op'] in (LT, LE):
        with np.errstate(invalid='ignore'):
            h = thresholds_of(thr, index, c['T'], c['E'])
            x = np.where(np.isfinite(h), h - (x - h), -x).astype(np.float32)
    return x, thr, index
