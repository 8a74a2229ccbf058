"""
The least-squares fit along the row axis (csrc/time_regression.hip, include/dlwpcs.h dlwpcs_time_regression) restated in numpy
float64 operation by operation: vectorised over the elements (fit_ref), and once more as an independent scalar walk over one
element (fit_scalar); the evaluation (apply_ref), the planner's table and the inputs.  Not a test module: imported by
test_time_regression_ref.py, test_time_regression.py (CPU) and test_gpu_time_regression.py.

Definition (the header's).  x: T rows of fp32, basis b: (T, K) fp32, slabs of S rows, min_count >= K, pivot_tol (0: 2^-40).  At
element e every operation is fp64, rounded once:
    1. row r is present when x[r, e] is not NaN (an infinity is a value)
    2. a slab starts from zero and takes its present rows in row order:  c[k] += b[r,k] x[r,e];  G[i][j] += b[r,i] b[r,j], j <= i;
       n += 1.  (fp32 factors: the products are exact, numpy's * and + give the bits of the device's fma)
    3. the slab sums are added to totals that start from zero, in slab order
    4. for j = 0 .. K-1:  s = 0; for p < j: s = s + (L[j][p] L[j][p]) d[p];  d[j] = G[j][j] - s;
       singular unless d[j] > pivot_tol G[j][j];  for i > j: s = 0; for p < j: s = s + (L[i][p] L[j][p]) d[p];
       L[i][j] = (G[i][j] - s) / d[j]
    5. z[i] = c[i] - sum_{p<i} L[i][p] z[p] (s from 0, p ascending);  w = z / d;  a[i] = w[i] - sum_{p>i} L[p][i] a[p], i descending,
       p ascending
    6. coef[k] = float32(a[k]); all K are QNAN (0x7fc00000) when n < min_count, the column is singular, a float32(a[k]) is not
       finite, or the mode is PROPAGATE and n < T
    7. count = n

Error against numpy.linalg.lstsq in fp64 on the present rows (test_time_regression_ref.py): half an ulp of the final rounding plus
the fp64 solve error.  Measured with the hostile recipe (10 % NaN), harmonic bases of K = 4, 6, 10, 16 and T = 40 .. 1100: at
most 0.96 x 2^-24 x max_k |coef_k| on every kept column (the cases of test_time_regression_ref.py: 0.941, 0.915, 0.956, 0.934,
0.915, 0.943); the test takes 2 x 2^-24 x max_k |coef_k|, the margin covers other seeds.

The planner, restated in plan():
    term class = the power of two >= K (1 .. 16).  16-byte chunks where the layout and the pointers allow them and the class is
    at most 8, else one element per lane.  tiles = ceil(chunks per row / 256), slabs = max(1, ceil(T / S)).
    split: what the caller forces, else slabs > 1 and tiles < 512.  gram: what the caller forces, else 0 (the shared factor).
    grid of the first launch over the rows = tiles x (slabs if split else 1) workgroups, as (min(n, 65536), ceil(n / 65536)).
"""
import numpy as np

QNAN = np.uint32(0x7fc00000)
SKIP, PROPAGATE = 0, 1
FITTED, RESIDUAL = 0, 1
MAX_TERMS = 16
SLAB_ROWS = 512
THREADS = 256
VEC_MAX_CLASS = 8
TARGET_BLOCKS = 512
PIVOT_TOL = 2.0 ** -40
U = 2.0 ** -24
MEASURED = 0.96                 # x 2^-24 x max |coef|: the largest error against lstsq seen (module docstring)

K_CASES = (1, 2, 3, 4, 5, 8, 9, 10, 16)
E_CASES = (1, 3, 4, 5, 255, 256, 257, 1028)


def term_class(K):
    c = 1
    while c < K:
        c *= 2
    return c


def plan(T, K, inner, vec_ok, slab_rows=0, split=-1, gram=-1):
    """(split, gram, class, chunk, grid, slab rows) of the planner for `inner` elements per row; vec_ok: the layout and the
    pointers allow 16-byte chunks.  None: refused."""
    if not 1 <= K <= MAX_TERMS or T < 0 or slab_rows < 0:
        return None
    S = slab_rows or SLAB_ROWS
    cls = term_class(K)
    vec = bool(vec_ok) and cls <= VEC_MAX_CLASS
    tiles = -(-(inner // (4 if vec else 1)) // THREADS)
    slabs = max(1, -(-T // S))
    sp = bool(split) if split >= 0 else (slabs > 1 and tiles < TARGET_BLOCKS)
    n = tiles * (slabs if sp else 1) if inner else 0
    gx = min(n, 65536)
    return (int(sp), 1 if gram == 1 else 0, cls, 4 if vec else 1, (gx, -(-n // gx)) if n else (0, 0), S)


# --------------------------------------------------------------------------------------------------------------------- #
# the definition, vectorised over elements
# --------------------------------------------------------------------------------------------------------------------- #

def _tri(K):
    return [(i, j) for i in range(K) for j in range(i + 1)]


def sums_ref(x, b, S):
    """steps 1 to 3 on x (T, E) float32, b (T, K) float32: (c (K, E), G (K, K, E) lower triangle, n (E,) int32) in float64"""
    x, b = np.asarray(x), np.asarray(b)
    assert x.dtype == np.float32 and b.dtype == np.float32 and x.ndim == 2 and b.ndim == 2 and b.shape[0] == x.shape[0]
    T, E = x.shape
    K = b.shape[1]
    bd = b.astype(np.float64)
    ii, jj = (np.array(v) for v in zip(*_tri(K)))
    c, Gp, n = np.zeros((K, E)), np.zeros((len(ii), E)), np.zeros(E, np.int32)
    with np.errstate(all='ignore'):
        for r0 in range(0, T, S):
            cs, Gs = np.zeros((K, E)), np.zeros((len(ii), E))
            for r in range(r0, min(r0 + S, T)):
                present = ~np.isnan(x[r])
                # an absent row adds b * 0 = +-0, which changes no sum that started at +0: the bits of adding nothing
                xz = np.where(present, x[r], np.float32(0)).astype(np.float64)
                cs = cs + bd[r][:, None] * xz[None, :]
                Gs = Gs + (bd[r, ii] * bd[r, jj])[:, None] * present[None, :]
                n += present
            c = c + cs
            Gp = Gp + Gs
    G = np.zeros((K, K, E))
    G[ii, jj] = Gp
    return c, G, n


def solve_ref(c, G, pivot_tol=0.):
    """steps 4 and 5, vectorised over the last axis: (a (K, E) float64, singular (E,) bool); a of a singular column is nan"""
    K, E = c.shape
    tol = pivot_tol or PIVOT_TOL
    L, d = np.zeros((K, K, E)), np.zeros((K, E))
    singular = np.zeros(E, bool)
    with np.errstate(all='ignore'):
        for j in range(K):
            s = np.zeros(E)
            for p in range(j):
                s = s + (L[j, p] * L[j, p]) * d[p]
            dj = G[j, j] - s
            singular |= ~(dj > tol * G[j, j])
            d[j] = np.where(singular, np.nan, dj)               # (nothing of a singular column is used)
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
    a[:, singular] = np.nan
    return a, singular


def fit_ref(x, b, mode=SKIP, min_count=None, pivot_tol=0., slab_rows=0):
    """the definition: (coef float32 (K, E), count int32 (E,), singular (E,) bool)"""
    x, b = np.asarray(x), np.asarray(b)
    T, K = b.shape
    mc = K if min_count is None else int(min_count)
    assert mc >= K
    c, G, n = sums_ref(x, b, slab_rows or SLAB_ROWS)
    a, singular = solve_ref(c, G, pivot_tol)
    with np.errstate(all='ignore'):
        coef = a.astype(np.float32)
    bad = (n < mc) | singular | ~np.all(np.isfinite(coef), axis=0)
    if mode == PROPAGATE:
        bad |= n < T
    bits = coef.view(np.uint32).copy()
    bits[:, bad] = QNAN
    return bits.view(np.float32), n, singular


def apply_ref(b, coef, x=None):
    """dlwpcs_time_regression_apply on b (R, K) float32, coef (K, E) float32: fitted values, or with x (R, E) the residuals"""
    b, coef = np.asarray(b), np.asarray(coef)
    assert b.dtype == np.float32 and coef.dtype == np.float32
    R, K = b.shape
    f = np.zeros((R, coef.shape[1]))
    with np.errstate(all='ignore'):
        for k in range(K):
            f = f + b[:, k].astype(np.float64)[:, None] * coef[k].astype(np.float64)[None, :]
        y = (f if x is None else np.asarray(x).astype(np.float64) - f).astype(np.float32)
    bad = np.isnan(coef).any(axis=0)[None, :] | np.isnan(y)
    bits = y.view(np.uint32).copy()
    bits[bad] = QNAN
    return bits.view(np.float32)


# --------------------------------------------------------------------------------------------------------------------- #
# the definition once more: one element, python floats, nothing shared with the above but the text of the header
# --------------------------------------------------------------------------------------------------------------------- #

def fit_scalar(xcol, b, mode=SKIP, min_count=None, pivot_tol=0., slab_rows=0):
    """(list of K uint32 bit patterns, n) of one column xcol (T,) float32"""
    T, K = b.shape
    S = slab_rows or SLAB_ROWS
    tol = pivot_tol or PIVOT_TOL
    mc = K if min_count is None else int(min_count)
    nanbits = [int(QNAN)] * K
    c = [0.0] * K
    G = [[0.0] * K for _ in range(K)]
    n = 0
    r = 0
    while r < T:
        cs = [0.0] * K
        Gs = [[0.0] * K for _ in range(K)]
        for rr in range(r, min(r + S, T)):
            xv = float(xcol[rr])
            if xv != xv:
                continue
            row = [float(v) for v in b[rr]]
            with np.errstate(all='ignore'):
                for k in range(K):
                    cs[k] = float(np.float64(cs[k]) + np.float64(row[k]) * np.float64(xv))
            for i in range(K):
                for j in range(i + 1):
                    Gs[i][j] += row[i] * row[j]
            n += 1
        with np.errstate(all='ignore'):
            for k in range(K):
                c[k] = float(np.float64(c[k]) + np.float64(cs[k]))
        for i in range(K):
            for j in range(i + 1):
                G[i][j] += Gs[i][j]
        r += S
    if n < mc or (mode == PROPAGATE and n < T):
        return nanbits, n
    L = [[0.0] * K for _ in range(K)]
    d = [0.0] * K
    with np.errstate(all='ignore'):
        for j in range(K):
            s = np.float64(0.)
            for p in range(j):
                s = s + (np.float64(L[j][p]) * np.float64(L[j][p])) * np.float64(d[p])
            dj = np.float64(G[j][j]) - s
            if not dj > np.float64(tol) * np.float64(G[j][j]):
                return nanbits, n
            d[j] = float(dj)
            for i in range(j + 1, K):
                s = np.float64(0.)
                for p in range(j):
                    s = s + (np.float64(L[i][p]) * np.float64(L[j][p])) * np.float64(d[p])
                L[i][j] = float((np.float64(G[i][j]) - s) / dj)
        z = [np.float64(0.)] * K
        for i in range(K):
            s = np.float64(0.)
            for p in range(i):
                s = s + np.float64(L[i][p]) * z[p]
            z[i] = np.float64(c[i]) - s
        w = [z[i] / np.float64(d[i]) for i in range(K)]
        a = [np.float64(0.)] * K
        for i in range(K - 1, -1, -1):
            s = np.float64(0.)
            for p in range(i + 1, K):
                s = s + np.float64(L[p][i]) * a[p]
            a[i] = w[i] - s
        out = [np.float32(v) for v in a]
    if not all(np.isfinite(v) for v in out):
        return nanbits, n
    return [int(np.array(v, np.float32).view(np.uint32)) for v in out], n


# --------------------------------------------------------------------------------------------------------------------- #
# inputs
# --------------------------------------------------------------------------------------------------------------------- #

def make_series(rng, T, E, K=0, hostile=True):
    """the recipe of time_filter_ref.make_series: (T, E) float32 around 270 +- 50; hostile: about 10 % NaN, a few +-inf and -0,
    one whole NaN column and one whole NaN row; plus (K > 1, E > 3, T >= K) one column with exactly K - 1 present rows"""
    x = (rng.normal(size=(T, E)) * 50. + 270.).astype(np.float32)
    if hostile and x.size:
        x[rng.random(x.shape) < 0.1] = np.nan
        for v in (np.inf, -np.inf, -0.0, np.inf):
            x[rng.integers(T), rng.integers(E)] = v
        if E > 2:
            x[:, rng.integers(E)] = np.nan
        if T > 2:
            x[rng.integers(T)] = np.nan
        if K > 1 and E > 3 and T >= K:
            col = int(rng.integers(E))
            keep = rng.choice(T, K - 1, replace=False)
            vals = (rng.normal(size=K - 1) * 50. + 270.).astype(np.float32)
            x[:, col] = np.nan
            x[keep, col] = vals
    return x


def harmonic_basis(T, K, period=None, trend=None):
    """(T, K) float32: 1, [a trend on [-1, 1] when K is even,] then cos and sin of the harmonics of `period` rows (default: T /
    2.3, a few cycles and no whole number of them)"""
    t = np.arange(T, dtype=np.float64)
    period = period or max(T, 2) / 2.3
    trend = (K % 2 == 0) if trend is None else trend
    cols = [np.ones(T)]
    if trend and K > 1:
        cols.append((2. * t - (T - 1)) / max(T - 1, 1))
    h = 1
    while len(cols) < K:
        ang = 2. * np.pi * h * t / period
        cols.append(np.cos(ang))
        if len(cols) < K:
            cols.append(np.sin(ang))
        h += 1
    return np.stack(cols, axis=1).astype(np.float32)
