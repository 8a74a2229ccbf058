"""
Reference and case tables of the time spectrum tests (test_time_spectrum_ref.py, test_time_spectrum.py,
test_gpu_time_spectrum.py).  Not a test module.

reference(): the definition of dlwpcs_time_spectrum (include/dlwpcs.h) in float64, written with plain loops per column and
segment, independently of DLWP.verify's vectorised numpy twin: the segment's mean is the fp64 sum in row order over M, rounded
to float32 (that rounding is part of the definition: y belongs to the rounded mean), y_t = w_t (x_t - mean) in float64 from the
float32 window, X = np.fft.rfft(y), P_f = c_f |X_f|^2 / (M S_w), the mean over the segments that are finite (in both operands).
It also returns the scales of the bounds: m = the mean over the counted segments of sum_t y_t^2 / S_w per operand and column, and
sum_t |y_t| per segment and column for the coefficient form.

bound(): derived, not tuned.  The device forms Re X_f and Im X_f as fp32 fma chains of length M.  Every term carries the rounding
of its twiddle (correctly rounded from fp64), of the window product and of the mean subtraction, 2^-24 each, and at most M
roundings of the chain: |dX_f| <= (M + 3) 2^-24 sum_t |y_t| <= (M + 3) 2^-24 sqrt(M) |y|_2, while |X_f| <= sqrt(M) |y|_2.  So
c_f (2 |X_f| |dX_f|) / (M S_w) <= 4 (M + 3) 2^-24 m.  The fp32 product fma(Im, Im, Re * Re) rounds twice (2 * 2^-24 * P_f <=
4 * 2^-24 m: one more unit of the constant), the stored fp32 result once (half a unit), the fp64 sums do not count.  With the
second-order terms this is
    |P - ref| <= 4 (M + C) 2^-24 m,     C = 6
(3 for the three roundings per term, 1 for the product, 0.5 for the result, 1.5 of slack for the second-order terms, which are
below M^2 2^-48 m).  Co and quad use sqrt(m_a m_b): the mean over segments of sqrt(m_a m_b) is at most that by Cauchy-Schwarz.
bound_coef(): |Re dX_f|, |Im dX_f| <= (M + C_COEF) 2^-24 sum_t |y_t| with C_COEF = 4 (the three roundings per term and the
second-order slack).  A device value outside these bounds is a bug in the kernel, not a reason to widen them.
"""
import numpy as np

EPS = 2.0 ** -24
C = 6.0
C_COEF = 4.0
MAX_M = 1728
SLAB = 8                                            # DLWPCS_TIME_SPECTRUM_SLAB_SEGMENTS
GPU_M = [2, 3, 4, 5, 8, 31, 32, 33, 63, 64, 65, 96, 129, 360]
COLUMNS = [1, 31, 32, 33, 257, 1028]
N_FREQ = [1, 2, 33, 129, None]
WINDOWS = ['boxcar', 'hann', 'random']
NAN_BITS = (0x7FC00000, 0x7FA00000, 0xFFC00000, 0xFF800001, 0x7F800000, 0xFF800000)       # spectrum_ref.NAN_BITS


def hops(M):
    return [1, max(M // 2, 1), M, M + 3]


def full_k(M):
    return M // 2 + 1


def clip_freq(n_freq, M):
    return full_k(M) if n_freq is None or n_freq >= full_k(M) else n_freq


def n_segments(T, M, hop):
    return (T - M) // hop + 1 if T >= M else 0


def rows_for(M, hop, n_seg=4):
    """rows for n_seg segments and, where the hop allows it, rows left over"""
    return M + (n_seg - 1) * hop + min(hop - 1, 2)


def c_f(M, K):
    c = np.full(K, 2.0)
    c[0] = 1.0
    if M % 2 == 0 and K == M // 2 + 1:
        c[K - 1] = 1.0
    return c


def window(kind, M, rng=None):
    """float32 window weights: each entry evaluated in float64 and rounded once"""
    if kind == 'boxcar':
        w = np.ones(M)
    elif kind == 'hann':
        w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(M, dtype=np.float64) / M)
    else:
        w = rng.uniform(-1.0, 1.0, M)
    return w.astype(np.float32)


def twiddle(M):
    ang = 2.0 * np.pi * np.arange(M, dtype=np.float64) / M
    return np.stack([np.cos(ang), -np.sin(ang)], axis=1).astype(np.float32)


def segment_mean32(seg):
    """the definition's mean of a (M,) float32 segment: the fp64 sum in row order over M, rounded to float32"""
    s = np.float64(0.0)
    for v in seg:
        s = s + np.float64(v)
    return np.float32(s / np.float64(len(seg)))


def reference(a, M, hop, w32, detrend, n_freq=None, min_count=1, b=None):
    """
    a, b: (T, C) float32.  Returns dict(power (nq, K, C) float64, count (C,) int32, m (2, C) float64, coef (n_seg, K, C)
    complex128 of a (NaN where the segment does not count in a), sum_abs (n_seg, C) float64 of a).
    """
    a = np.asarray(a, dtype=np.float32)
    pair = b is not None
    ops = [a, np.asarray(b, dtype=np.float32)] if pair else [a]
    T, ncol = a.shape
    K = clip_freq(n_freq, M)
    n_seg = n_segments(T, M, hop)
    w = np.asarray(w32, dtype=np.float32).astype(np.float64)
    sw = float((w ** 2).sum())
    scale = c_f(M, K) / (M * sw)
    nq = 4 if pair else 1
    power = np.full((nq, K, ncol), np.nan)
    count = np.zeros(ncol, dtype=np.int32)
    m = np.full((2, ncol), np.nan)
    coef = np.full((n_seg, K, ncol), complex(np.nan, np.nan), dtype=np.complex128)
    sum_abs = np.full((n_seg, ncol), np.nan)
    for c in range(ncol):
        acc, accm, n = np.zeros((nq, K)), np.zeros(2), 0
        for s in range(n_seg):
            X, ok = [], True
            for i, x in enumerate(ops):
                seg = x[s * hop:s * hop + M, c]
                fin = bool(np.isfinite(seg).all())
                ok = ok and fin
                if not fin:
                    X.append(None)
                    continue
                mu = np.float64(segment_mean32(seg)) if detrend else 0.0
                y = w * (seg.astype(np.float64) - mu)
                X.append((np.fft.rfft(y)[:K], float((y ** 2).sum()) / sw))
                if i == 0:
                    coef[s, :, c] = X[0][0]
                    sum_abs[s, c] = np.abs(y).sum()
            if not ok:
                continue
            A, B = X[0][0], X[-1][0]
            q = [A.real ** 2 + A.imag ** 2]
            if pair:
                cr = A * np.conj(B)
                q += [B.real ** 2 + B.imag ** 2, cr.real, cr.imag]
            acc += np.array(q)
            accm += np.array([X[0][1], X[-1][1]])
            n += 1
        count[c] = n
        if n >= max(min_count, 1):
            power[:, :, c] = acc * scale / n
            m[:, c] = accm / n
    return dict(power=power, count=count, m=m, coef=coef, sum_abs=sum_abs)


def bound(M, m, nq):
    """(nq, 1, C): the largest allowed |device - reference| per quantity, for every frequency"""
    b = 4.0 * (M + C) * EPS
    if nq == 1:
        return b * m[:1, None, :]
    g = np.sqrt(m[0] * m[1])
    return b * np.stack([m[0], m[1], g, g])[:, None, :]


def bound_coef(M, sum_abs):
    """(n_seg, 1, C): the largest allowed |device - reference| of Re X_f and of Im X_f"""
    return (M + C_COEF) * EPS * sum_abs[:, None, :]


def float32_restatement(a, M, hop, w32, detrend, n_freq=None):
    """the kernel's arithmetic on the host for the single form: fp32 mean subtraction and window product, fp32 fma chains in row
    order against the float32 twiddle table at (f t) mod M (the fma as an exact float64 product and sum rounded to float32), the
    fp32 product fma(Im, Im, Re * Re) widened to fp64 and summed.  Finite input.  (power (K, C), coef (n_seg, K, C))"""
    a = np.asarray(a, dtype=np.float32)
    T, ncol = a.shape
    K = clip_freq(n_freq, M)
    n_seg = n_segments(T, M, hop)
    tw = twiddle(M).astype(np.float64)
    w32 = np.asarray(w32, dtype=np.float32)
    sw = float((w32.astype(np.float64) ** 2).sum())
    f = np.arange(K)
    coef = np.zeros((n_seg, K, ncol), dtype=np.complex128)
    total = np.zeros((K, ncol))
    for s in range(n_seg):
        seg = a[s * hop:s * hop + M]
        mu = np.array([segment_mean32(seg[:, c]) for c in range(ncol)], dtype=np.float32) if detrend else np.zeros(ncol, np.float32)
        y = (w32[:, None] * (seg - mu[None, :]).astype(np.float32)).astype(np.float32)
        re = np.zeros((K, ncol), dtype=np.float32)
        im = np.zeros((K, ncol), dtype=np.float32)
        for t in range(M):
            idx = (f * t) % M
            yt = y[t].astype(np.float64)[None, :]
            re = (re.astype(np.float64) + tw[idx, 0][:, None] * yt).astype(np.float32)
            im = (im.astype(np.float64) + tw[idx, 1][:, None] * yt).astype(np.float32)
        coef[s] = re.astype(np.float64) + 1j * im.astype(np.float64)
        rr = (re.astype(np.float64) * re.astype(np.float64)).astype(np.float32)
        p = (im.astype(np.float64) * im.astype(np.float64) + rr.astype(np.float64)).astype(np.float32)
        total += p.astype(np.float64)
    scale = c_f(M, K) / (M * sw)
    return (total * scale[:, None] / max(n_seg, 1)).astype(np.float32).astype(np.float64), coef


def make_series(rng, T, ncol, offset=0.0):
    """red-ish noise per column with unequal amplitudes: (T, ncol) float32"""
    x = rng.standard_normal((T, ncol))
    x[1:] += 0.6 * x[:-1]
    return (offset + x * rng.uniform(0.5, 2.0, ncol)[None, :]).astype(np.float32)


def direct_dft(y, K):
    """the O(M^2) sum X_f = sum_t y_t exp(-2 pi i f t / M) in float64 with the angle reduced in integers"""
    M = len(y)
    t = np.arange(M)
    return np.array([(y * np.exp(-2j * np.pi * ((f * t) % M) / M)).sum() for f in range(K)])
