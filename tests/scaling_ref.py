"""
numpy references of the per-variable scaling kernels (include/dlwpcs.h, dlwpcs_channel_moments / dlwpcs_channel_affine), shared by
tests/test_scaling.py and tests/test_gpu_scaling.py.  Arrays are addressed as (R rows, C channels, S inner elements).
"""
import numpy as np

MUL_ADD, SUB_DIV = 0, 1
U53 = 2.0 ** -53


def moments(x, rows=None, center=None, skipna=False):
    """x (R, C, S) float32 -> (C, 3) float64 {n, sum (x - center), sum (x - center)^2} over the rows in `rows` (None: all; duplicates
    count as given), the difference formed in fp64.  skipna: NaN elements are left out of all three, else they propagate."""
    x = np.asarray(x)
    assert x.ndim == 3 and x.dtype == np.float32
    if rows is not None:
        x = x[np.asarray(rows, dtype=np.int64)]
    C = x.shape[1]
    out = np.zeros((C, 3), dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        for c in range(C):
            d = x[:, c, :].astype(np.float64).reshape(-1)
            if center is not None:
                d = d - float(center[c])
            if skipna:
                d = d[~np.isnan(d)]
            out[c] = (d.size, d.sum(), (d * d).sum())
    return out


def moments_bound(x, rows=None, center=None):
    """(C, 3) a-priori bounds on |device - moments()|: 0 for the count; for a sum of n fp64 terms t_i added in ANY order,
    n * 2^-53 * sum |t_i| (every partial sum is at most sum |t_i| and each of the n - 1 additions rounds once; the one rounding of
    a square, or none under an fma, is covered by the same figure).  NaN terms are left out of the bound's own sums."""
    x = np.asarray(x)
    if rows is not None:
        x = x[np.asarray(rows, dtype=np.int64)]
    C = x.shape[1]
    out = np.zeros((C, 3), dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        for c in range(C):
            d = x[:, c, :].astype(np.float64).reshape(-1)
            if center is not None:
                d = d - float(center[c])
            d = d[~np.isnan(d)]
            out[c] = (0.0, d.size * U53 * np.abs(d).sum(), d.size * U53 * (d * d).sum())
    return out


def affine(x, a, b, mode, axis=1):
    """float32, two roundings: x * a[c] + b[c] (MUL_ADD) or (x - b[c]) / a[c] (SUB_DIV), c the index along `axis`"""
    x = np.asarray(x)
    assert x.dtype == np.float32
    shape = [1] * x.ndim
    shape[axis] = x.shape[axis]
    a = np.asarray(a, dtype=np.float32).reshape(shape)
    b = np.asarray(b, dtype=np.float32).reshape(shape)
    with np.errstate(all='ignore'):
        if mode == MUL_ADD:
            y = x * a
            y = y + b
        else:
            y = x - b
            y = y / a
    assert y.dtype == np.float32
    return y


def same_bits(got, want):
    """bitwise equal, a NaN matching any NaN (IEEE 754 leaves the sign and payload of a generated NaN open)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != np.float32 or want.dtype != np.float32:
        return False
    return bool(np.all((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))


# (row, channel, inner) element strides of the layouts under test, for an (R, C, S) array
def strides_channels_first(R, C, S):
    return (C * S, S, 1)


def strides_channels_last(R, C, S):
    return (S * C, 1, C)


def strides_channels_last_folded(R, C, S):
    """the row extent folded into S: R = 1, S <- R * S"""
    return (0, 1, C)
