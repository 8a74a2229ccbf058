"""
Reference, case tables and error bound of the lagged-covariance tests (test_time_lag_ref.py, test_gpu_time_lag.py,
test_gpu_time_lag_verify.py).  Not a test module.

reference(): the definition of dlwpcs_time_lag (include/dlwpcs.h) restated in numpy, bit for bit: the deviations are ONE float32
subtraction (a missing entry: +0), the products are float64 (exact: 24 x 24 bits fit in 53), a slab of SLAB = 512 a rows is
summed row by row from +0 (np.cumsum is sequential), the slab sums are added in slab order from +0, the value is one float64
division rounded to float32 once, every NaN is 0x7fc00000, the counts are the pairs with both entries present.  split=True keeps
the slab sums of every lag in an array first and adds them afterwards (the two-launch form), split=False adds every slab sum to
the total as soon as it is finished (the walking lane): the same additions.  reference_loops() is the same statement with plain
Python loops per column, lag, slab and row, for small cases.

bound(): |device value - exact value| for the covariance with centre 'mean', where the exact value is the float64 definition
with the exact mean m over the rows present (what DLWP.verify computes on the host) and the device value is reference() with the
float32 centre of ops.group_mean.  Derived, not tuned; n is the number of pairs of the lag, the sums run over those pairs, da and
db are the exact deviations:
  1. The centre.  group_mean adds the rows in float64 and rounds once: |m~ - m| <= dm = 2^-24 |m| + n_rows 2^-53 mean|x| (the
     second term is the float64 chain of the sum).  Replacing m by m~ moves every deviation by at most dm, so a product moves
     by at most |da| dm_b + |db| dm_a + dm_a dm_b.
  2. The subtraction.  fl(a - m~) carries one float32 rounding, relative 2^-24, on each factor: the product moves by at most
     |da'| |db'| (2^-23 + 2^-48), with da' the deviations from m~, |da'| <= |da| + dm_a.
  3. The chain.  n float64 additions of exact products: at most n 2^-53 sum |da' db'|.
  4. The result.  One division in float64 (2^-53, inside the slack of 3.) and one rounding to float32: 2^-24 |c|.
So  |c~ - c| <= [ sum (|da'| |db'| (2^-23 + 2^-48) + |da| dm_b + |db| dm_a + dm_a dm_b) + 3 (n + 1) 2^-53 sum |da' db'| ] / n
                 + 2^-24 (|c| + the bracket),
the factor 3 on the chain covering the float64 sums of the host twin the device is compared with (numpy's own order) as well.
The verify-level test carries this bound through the quotients of the derived functions to first order, with one 2^-24 per
float32 operation of the device path (test_gpu_time_lag_verify.py states each).
On the verify cases (AR(1), phi = 0.8, standard deviation 100 on an offset of 5500: geopotential height in metres) the centre
term dominates: 2 E|d| dm / var = 2 * 80 * 3.3e-4 / 1e4 = 5e-6 of the variance; test_time_lag_ref.py holds the bound below 1e-5
of the lag-0 variance there, so that it cannot hide a wrong kernel.
"""
import numpy as np

SLAB = 512                                          # DLWPCS_TIME_LAG_SLAB_ROWS
MAX_LAGS = 1024
SKIP, PROPAGATE = 0, 1
QNAN = np.uint32(0x7fc00000)
BLOCKS = (1, 4, 8, 16)                              # the accumulator classes of the kernel; a pass serves up to 16 lags

ROWS = [1, 2, 511, 512, 513, 1025]
COLUMNS = [1, 3, 4, 257, 1028]
NAN_PATTERNS = ['none', 'one percent', 'column', 'slab edge', 'b only']
MODES = [(SKIP, 1), (SKIP, 5), (PROPAGATE, 1)]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def lag_sets(T, widths=BLOCKS):
    """{name: lags}: every set the device test runs at T rows; each has a lag with pairs, and (but [0]) one without"""
    sets = {'zero': [0], 'both sides': list(range(-9, 10)), 'step 4': list(range(-8, 13, 4)),
            'the ends': [T - 1, T, T + 1], 'the ends, backwards': [-T - 1, -T, -T + 1]}
    for w in widths:
        for L in (w - 1, w, w + 1):
            if L >= 1:
                sets['0..%d' % L] = list(range(0, L + 1))
    if T == 1025:
        sets['longer than a slab'] = [600]
    return sets


def make_series(rng, T, E, pattern='none', offset=250.0, scale=5.0):
    """(a, b) float32 (T, E): red noise on an offset; the NaN pattern goes into a (and, but for 'b only', into b at other places)"""
    def red():
        x = rng.standard_normal((T, E))
        for t in range(1, T):
            x[t] += 0.7 * x[t - 1]
        return (x * scale + offset).astype(np.float32)
    a, b = red(), red()
    if pattern == 'one percent':
        a[rng.random((T, E)) < 0.01] = np.nan
        b[rng.random((T, E)) < 0.01] = np.nan
    elif pattern == 'column':
        a[:, E // 2] = np.nan
        b[T // 2:, 0] = np.nan
    elif pattern == 'slab edge':
        for t in (SLAB - 1, SLAB):
            if t < T:
                a[t, ::2] = np.nan
                b[t, 1::3] = np.nan
        a[0, 0] = np.nan
        a[T - 1, E - 1] = np.nan
    elif pattern == 'b only':
        b[rng.random((T, E)) < 0.05] = np.nan
    elif pattern != 'none':
        raise KeyError(pattern)
    return a, b


def centre(x):
    """the float32 centre of a (T, E) or (T,) series as ops.group_mean with one group gives it: the float64 sum of the rows present
    in row order inside slabs of 512 rows, the slab sums in slab order, over the count, rounded once; NaN where no row is present"""
    x = np.asarray(x, dtype=np.float32)
    v = x.reshape(x.shape[0], -1).astype(np.float64)
    ok = ~np.isnan(v)
    tot = np.zeros(v.shape[1])
    for r0 in range(0, v.shape[0], SLAB):
        z = np.where(ok[r0:r0 + SLAB], v[r0:r0 + SLAB], 0.0)
        tot = tot + np.cumsum(np.concatenate([np.zeros((1, v.shape[1])), z]), axis=0)[-1]
    n = ok.sum(axis=0)
    with np.errstate(invalid='ignore', divide='ignore'):
        m = np.where(n > 0, tot / np.maximum(n, 1), np.nan).astype(np.float32)
    return m.reshape(x.shape[1:])


def deviations(x, c):
    """(float64 deviations of ONE float32 subtraction, presence) of a float32 series and its float32 centre (None: nothing)"""
    x = np.asarray(x, dtype=np.float32)
    present = ~np.isnan(x)
    with np.errstate(invalid='ignore', over='ignore'):
        d = x if c is None else (x - np.asarray(c, dtype=np.float32)).astype(np.float32)
    assert d.dtype == np.float32
    return np.where(present, d, np.float32(0.0)).astype(np.float64), present


def need(T, lag, mode, min_count):
    return max(T - abs(lag), 1) if mode == PROPAGATE else max(min_count, 1)


def value(S, n, T, lag, mode, min_count):
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        v = (S / n.astype(np.float64)).astype(np.float32)
    out = bits(v).copy()
    out[np.isnan(v) | (n < need(T, lag, mode, min_count))] = QNAN
    return out.view(np.float32)


def _operands(a, b, ca, cb):
    a = np.asarray(a, dtype=np.float32)
    assert a.ndim == 2
    da, pa = deviations(a, ca)
    if b is None:
        db, pb = (da, pa) if cb is None else deviations(a, cb)
    else:
        b = np.asarray(b, dtype=np.float32)
        db, pb = deviations(b, cb)
        if b.ndim == 1:
            db, pb = db[:, None], pb[:, None]
    return a.shape[0], a.shape[1], da, pa, db, pb


def reference(a, b, lags, ca=None, cb=None, mode=SKIP, min_count=1, split=False):
    """a (T, E) float32; b None (auto; cb None: ca), (T, E) (pair) or (T,) (index); ca (E,) float32, cb (E,) or one value, None:
    nothing is subtracted -> (values float32 (lags, E), counts int32 (lags, E))"""
    T, E, da, pa, db, pb = _operands(a, b, ca, cb)
    n_slab = -(-T // SLAB)
    out = np.empty((len(lags), E), dtype=np.float32)
    cnt = np.zeros((len(lags), E), dtype=np.int32)
    part = np.zeros((n_slab, len(lags), E))
    with np.errstate(invalid='ignore', over='ignore'):
        for i, l in enumerate(int(x) for x in lags):
            total = np.zeros(E)
            for s in range(n_slab):
                t0, t1 = max(s * SLAB, -l, 0), min((s + 1) * SLAB, T - l, T)
                run = np.zeros(E)
                if t1 > t0:
                    prod = da[t0:t1] * db[t0 + l:t1 + l]
                    run = np.cumsum(np.concatenate([np.zeros((1, E)), np.broadcast_to(prod, (t1 - t0, E))]), axis=0)[-1]
                    cnt[i] += (pa[t0:t1] & pb[t0 + l:t1 + l]).sum(axis=0).astype(np.int32)
                if split:
                    part[s, i] = run
                else:
                    total = total + run
            if split:
                for s in range(n_slab):
                    total = total + part[s, i]
            out[i] = value(total, cnt[i], T, l, mode, min_count)
    return out, cnt


def reference_loops(a, b, lags, ca=None, cb=None, mode=SKIP, min_count=1):
    """reference() with plain loops: per column, lag, slab and row"""
    T, E, da, pa, db, pb = _operands(a, b, ca, cb)
    db, pb = np.broadcast_to(db, (T, E)), np.broadcast_to(pb, (T, E))
    out = np.empty((len(lags), E), dtype=np.float32)
    cnt = np.zeros((len(lags), E), dtype=np.int32)
    with np.errstate(invalid='ignore', over='ignore'):
        for i, l in enumerate(int(x) for x in lags):
            S = np.zeros(E)
            for e in range(E):
                total, n = 0.0, 0
                for r0 in range(0, T, SLAB):
                    run = 0.0
                    for t in range(r0, min(r0 + SLAB, T)):
                        if 0 <= t + l < T:
                            run = run + da[t, e] * db[t + l, e]
                            n += int(pa[t, e] and pb[t + l, e])
                    total = total + run
                S[e], cnt[i, e] = total, n
            out[i] = value(S, cnt[i], T, l, mode, min_count)
    return out, cnt


def naive(a, b, lags, ca=None, cb=None, mode=SKIP, min_count=1):
    """the covariance in float64 with float64 deviations and numpy's own sums: (values float64, counts)"""
    a = np.asarray(a, dtype=np.float64)
    T, E = a.shape
    bb = a if b is None else np.asarray(b, dtype=np.float64)
    if bb.ndim == 1:
        bb = np.broadcast_to(bb[:, None], (T, E))
    cb = ca if (b is None and cb is None) else cb
    pa, pb = ~np.isnan(a), ~np.isnan(bb)
    with np.errstate(invalid='ignore'):
        da = np.where(pa, a - (0.0 if ca is None else np.asarray(ca, dtype=np.float64)), 0.0)
        db = np.where(pb, bb - (0.0 if cb is None else np.asarray(cb, dtype=np.float64)), 0.0)
    out = np.full((len(lags), E), np.nan)
    cnt = np.zeros((len(lags), E), dtype=np.int32)
    for i, l in enumerate(int(x) for x in lags):
        t0, t1 = max(0, -l), min(T, T - l)
        if t1 <= t0:
            continue
        n = (pa[t0:t1] & pb[t0 + l:t1 + l]).sum(axis=0)
        cnt[i] = n
        with np.errstate(invalid='ignore', divide='ignore'):
            out[i] = np.where(n >= need(T, l, mode, min_count), (da[t0:t1] * db[t0 + l:t1 + l]).sum(axis=0) / np.maximum(n, 1), np.nan)
    return out, cnt


# --------------------------------------------------------------------------------------------------------------------- #
# the verify-level cases and the bound
# --------------------------------------------------------------------------------------------------------------------- #

AR1_PHI, AR1_STD, AR1_OFFSET = 0.8, 100.0, 5500.0


def ar1(rng, T, E, phi=AR1_PHI, std=AR1_STD, offset=AR1_OFFSET, nan_fraction=0.0):
    """float32 (T, E): AR(1) columns of standard deviation `std` on `offset`"""
    x = np.empty((T, E))
    x[0] = rng.standard_normal(E)
    s = np.sqrt(1.0 - phi * phi)
    for t in range(1, T):
        x[t] = phi * x[t - 1] + s * rng.standard_normal(E)
    x = (x * std + offset).astype(np.float32)
    if nan_fraction:
        x[rng.random((T, E)) < nan_fraction] = np.nan
    return x


def centre_error(x):
    """dm of the docstring for a (T, E) or (T,) float32 series: (exact float64 mean, bound on |float32 centre - mean|)"""
    v = np.asarray(x, dtype=np.float64).reshape(np.shape(x)[0], -1)
    ok = ~np.isnan(v)
    n = np.maximum(ok.sum(axis=0), 1)
    m = np.where(ok, v, 0.0).sum(axis=0) / n
    mean_abs = np.where(ok, np.abs(v), 0.0).sum(axis=0) / n
    return m, 2.0 ** -24 * np.abs(m) + n * 2.0 ** -53 * mean_abs


def bound(a, b, lags):
    """(exact covariance float64 (lags, E), bound (lags, E)) for centre 'mean' (the docstring); NaN where a lag has no pairs"""
    a = np.asarray(a, dtype=np.float64)
    T, E = a.shape
    bb = a if b is None else np.asarray(b, dtype=np.float64)
    ma, dma = centre_error(a)
    mb, dmb = (ma, dma) if b is None else centre_error(bb)
    if bb.ndim == 1:
        bb = np.broadcast_to(bb[:, None], (T, E))
    pa, pb = ~np.isnan(a), ~np.isnan(bb)
    da, db = np.where(pa, a - ma, 0.0), np.where(pb, bb - mb, 0.0)
    exact = np.full((len(lags), E), np.nan)
    lim = np.full((len(lags), E), np.nan)
    u, u2 = 2.0 ** -23 + 2.0 ** -48, 2.0 ** -53
    for i, l in enumerate(int(x) for x in lags):
        t0, t1 = max(0, -l), min(T, T - l)
        if t1 <= t0:
            continue
        both = pa[t0:t1] & pb[t0 + l:t1 + l]
        n = np.maximum(both.sum(axis=0), 1)
        xa, xb = np.abs(da[t0:t1]), np.abs(db[t0 + l:t1 + l])
        moved = np.where(both, (xa + dma) * (xb + dmb), 0.0).sum(axis=0)
        centre_term = np.where(both, xa * dmb + xb * dma + dma * dmb, 0.0).sum(axis=0)
        c = (da[t0:t1] * db[t0 + l:t1 + l]).sum(axis=0) / n
        bracket = (moved * u + centre_term + 3 * (n + 1) * u2 * moved) / n       # (3: the chain, and twice that for a float64 twin's own sums)
        exact[i] = np.where(both.sum(axis=0) > 0, c, np.nan)
        lim[i] = bracket + 2.0 ** -24 * (np.abs(c) + bracket)
    return exact, lim
