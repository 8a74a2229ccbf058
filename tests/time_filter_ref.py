"""
The filter along the row axis (csrc/time_filter.hip, include/dlwpcs.h dlwpcs_time_filter) restated in numpy float32 operation by
operation, its fp64 expectation with the error bounds, the planner's table, and the inputs.  Not a test module: imported by
test_time_filter_ref.py, test_time_filter.py (CPU) and test_gpu_time_filter.py.

Definition (the header's).  T rows, taps h[0..K-1], step s, origin o; output row j at element e, in fp32, each operation rounded
once, in this order, no contraction:
    acc = 0; w = 0; n = 0; bad = False
    for k in 0 .. K-1:   r = j s + k - o
        missing = r < 0 or r >= T or isnan(x[r, e])
        missing:  bad = True                         (nothing is added)
        else:     acc = acc + h[k] * x[r, e];  w = w + h[k];  n = n + 1
    SUM (0):  out = QNAN if bad or isnan(acc) else acc
    MEAN (1): q = acc / w;  out = q if n > 0 and w >= min_weight and not isnan(q) else QNAN
QNAN = 0x7fc00000.  The kernel performs exactly these additions in tap order in both of its forms, so the tests compare bits.

Error bounds against exact arithmetic on the same float32 inputs (u = 2^-24, gamma_m = m u / (1 - m u), Higham 2002, 3.1 / 3.4; no
subnormals in the data, so every operation has relative error <= u):
    SUM:   K products and K additions; term k passes through its product and at most K additions (the first addition, to +0, is
           exact), K roundings:  |out - exact| <= gamma_K sum |h_k x_k|.
    MEAN:  numerator as above, gamma_K; the denominator w is a sum of K positive terms, relative error gamma_(K-1); the quotient
           one more rounding.  (1 + gamma_K)(1 + u) / (1 - gamma_(K-1)) - 1 <= gamma_(2K+1):
           |out - exact| <= gamma_(2K+1) sum_present |h_k x_k| / sum_present h_k.

The planner, restated in plan():
    A = ceil(K / s) live outputs per row.  form: streaming where A <= 8, else gather (forced: streaming up to A = 32, beyond
    it is refused).  class = the power of two >= A (1 .. 32), 0 in the gather form.
    16-byte chunks: where the layout and the pointers allow them (the last dim has source stride 1, every extent, stride and
    pointer keeps 16 bytes) and, streaming, class <= 8; else one element per lane.
    slab length (output rows): what the caller forces, else L = ceil(J / n) with n = min(ceil(1024 / tiles), J // Lmin), at
    least 1, Lmin = 8 class (streaming) or 8 (gather); tiles = ceil(chunks per row / 256).  Never more than J.
    grid = tiles x ceil(J / L) workgroups, as (min(n, 65536), ceil(n / 65536)).  No LDS.
"""
import numpy as np

QNAN = np.uint32(0x7fc00000)
SUM, MEAN = 0, 1
STREAMING, GATHER = 0, 1
MAX_TAPS = 4096
MAX_CLASS = 32
AUTO_MAX_CLASS = 8
VEC_MAX_CLASS = 8
THREADS = 256
TARGET_BLOCKS = 1024
U = 2.0 ** -24

# (K, s) pairs: every accumulator class, both sides of each class boundary, beyond the last; K < s, K = A s exactly
KS_CASES = ((1, 1), (1, 28), (2, 1), (2, 2), (3, 1), (3, 4), (4, 1), (5, 1), (5, 2), (8, 1), (8, 2), (9, 1), (9, 2), (16, 1), (16, 4),
            (17, 1), (17, 3), (28, 1), (28, 4), (28, 7), (28, 28), (32, 1), (32, 2), (33, 1), (33, 2), (33, 3), (61, 1), (61, 2), (61, 3),
            (61, 7), (61, 28))
E_CASES = (1, 3, 4, 5, 255, 256, 257, 1028)


def gamma(m):
    return m * U / (1. - m * U)


def n_live(K, s):
    return 1 if s >= K else -(-K // s)


def plan(K, s, J, inner, vec_ok, form=-1, slab_rows=0):
    """(form, class, vec, slab_rows, grid) of the planner for `inner` elements per row; vec_ok: the layout and the pointers allow
    16-byte chunks.  None: refused."""
    A = n_live(K, s)
    if form == STREAMING and A > MAX_CLASS:
        return None
    f = form if form >= 0 else (STREAMING if A <= AUTO_MAX_CLASS else GATHER)
    cls = 0
    if f == STREAMING:
        cls = 1
        while cls < A:
            cls *= 2
    vec = bool(vec_ok) and not (f == STREAMING and cls > VEC_MAX_CLASS)
    tiles = -(-(inner // (4 if vec else 1)) // THREADS)
    if slab_rows > 0:
        L = slab_rows
    else:
        lmin = 8 * cls if f == STREAMING else 8
        want = -(-TARGET_BLOCKS // tiles) if tiles else 1
        L = -(-J // max(1, min(want, J // lmin)))
    L = max(L, 1)
    if J > 0:
        L = min(L, J)
    n = tiles * (-(-J // L)) if J and inner else 0
    gx = min(n, 65536)
    return (f, cls, vec, L, (gx, -(-n // gx)) if n else (0, 0))


# --------------------------------------------------------------------------------------------------------------------- #
# the definition in float32, and in exact (fp64) arithmetic
# --------------------------------------------------------------------------------------------------------------------- #

def filter_ref(x, h, s, o, J, mode, min_weight=0.):
    """the definition on x (T, E) float32 with taps h float32: (out float32 (J, E), count int32 (J, E)); vectorised over j and
    e, the taps in order"""
    x, h = np.asarray(x), np.asarray(h)
    assert x.dtype == np.float32 and h.dtype == np.float32 and x.ndim == 2
    T, E = x.shape
    f = np.float32
    acc, w = np.zeros((J, E), f), np.zeros((J, E), f)
    n, bad = np.zeros((J, E), np.int32), np.zeros((J, E), bool)
    j = np.arange(J, dtype=np.int64)
    with np.errstate(all='ignore'):
        for k in range(len(h)):
            r = j * s + k - o
            inside = (r >= 0) & (r < T)
            v = x[np.clip(r, 0, max(T - 1, 0))] if T else np.full((J, E), np.nan, f)
            miss = ~inside[:, None] | np.isnan(v)
            p = (h[k] * v).astype(f)
            acc = np.where(miss, acc, (acc + p).astype(f))
            w = np.where(miss, w, (w + h[k]).astype(f))
            n += ~miss
            bad |= miss
        if mode == SUM:
            keep = ~(bad | np.isnan(acc))
            res = acc
        else:
            res = (acc / w).astype(f)
            keep = (n > 0) & (w >= f(min_weight)) & ~np.isnan(res)
    out = np.where(keep, res, f(0)).astype(f)
    bits = out.view(np.uint32).copy()
    bits[~keep] = QNAN
    return bits.view(f), n


def filter_exact(x, h, s, o, J):
    """fp64 on the same inputs: (sum over the present of h x, of |h x|, of h, count present, count of taps inside and present
    == K)"""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    T, E = x.shape
    num, ab, den = np.zeros((J, E)), np.zeros((J, E)), np.zeros((J, E))
    n = np.zeros((J, E), np.int64)
    j = np.arange(J, dtype=np.int64)
    with np.errstate(all='ignore'):
        for k in range(len(h)):
            r = j * s + k - o
            inside = (r >= 0) & (r < T)
            v = x[np.clip(r, 0, max(T - 1, 0))] if T else np.full((J, E), np.nan)
            ok = inside[:, None] & ~np.isnan(v)
            vz = np.where(ok, v, 0.)
            num += h[k] * vz
            ab += np.abs(h[k] * vz)
            den += np.where(ok, h[k], 0.)
            n += ok
    return num, ab, den, n


def bound_sum(K, ab):
    return gamma(K) * ab


def bound_mean(K, ab, den):
    with np.errstate(all='ignore'):
        return gamma(2 * K + 1) * ab / den


def fp32_sum(h):
    s = np.float32(0.)
    for v in np.asarray(h, dtype=np.float32):
        s = np.float32(s + v)
    return s


# --------------------------------------------------------------------------------------------------------------------- #
# inputs
# --------------------------------------------------------------------------------------------------------------------- #

def make_series(rng, T, E, hostile=True):
    """(T, E) float32 around 270 +- 50 (no subnormals); hostile: about 10 % NaN, a few +-inf and -0, one whole NaN column and
    one whole NaN row"""
    x = (rng.normal(size=(T, E)) * 50. + 270.).astype(np.float32)
    if hostile and x.size:
        x[rng.random(x.shape) < 0.1] = np.nan
        for v in (np.inf, -np.inf, -0.0, np.inf):
            x[rng.integers(T), rng.integers(E)] = v
        if E > 2:
            x[:, rng.integers(E)] = np.nan
        if T > 2:
            x[rng.integers(T)] = np.nan
    return x


def make_taps(rng, K, positive=False):
    """K float32 taps in (0.05, 1) (positive) or of both signs, none zero"""
    h = rng.random(K) * 0.95 + 0.05
    if not positive:
        h *= np.where(rng.random(K) < 0.4, -1., 1.)
    return h.astype(np.float32)


def n_out(T, K, s, mode):
    return max(0, (T - K) // s + 1) if mode == 'valid' else -(-T // s)
