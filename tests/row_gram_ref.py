"""
Reference and case tables of the row Gram tests (test_row_gram_ref.py, test_gpu_row_gram.py, test_gpu_eof.py).  Not a test module.

reference(): the definition of dlwpcs_row_gram (include/dlwpcs.h), independently of DLWP.verify's numpy twin.  Per column the
own mean is the fp64 sum of the rows in row order over the row count, rounded to float32 (the anomalies belong to the rounded
mean); y = fl(r * fl(x - mean)) in float32, one rounding per operation; a column is excluded where a value of a or of b or its
weight root is not finite (exponent all ones) or a given mean is NaN.  It returns the Gram matrix of those float32 y in float64
(a product of two float32 is exact in float64, and the fp64 sums of at most 2^15 such terms err by 2^-38 of the bound's scale:
"exact" for this purpose) and the diagonals of the two operands' own Gram matrices, the scales of the bound.

bound(): derived, not tuned.  Against that reference the device differs by the roundings of its fp32 chains only: within a slab
of S = 512 columns the value of (s, t) is an fmaf chain of at most S terms, whose error is at most gamma_S sum_slab |y_a[s] y_b[t]|
with gamma_S = S u / (1 - S u), u = 2^-24.  The slabs cover disjoint columns and the fp64 sums of the slab sums do not count, so by
Cauchy-Schwarz over all columns
    |G - ref|[s, t] <= (S + C) 2^-24 sqrt(ref_aa[s, s] ref_bb[t, t]),     C = 6
C is counted like C of time_spectrum_ref.py: 4 for the two roundings per factor (the subtraction and the weight product), which
a reference that did not round y would see, and 2 of slack for the second-order terms (S^2 u^2 = 2^-30 of the scale); with this
reference the 4 are slack as well.  A device value outside the bound is a bug in the kernel, not a reason to widen it.

emulate(): the slab / group order in numpy: per slab an fp32 chain over its columns in q order (the product exact in float64, the
sum rounded to float32: a double rounding stands in for the fma, which is why emulate makes no claim to the device's bits), the
slab sums added in float64 in slab order within groups of 16, the group sums in group order.
"""
import numpy as np

EPS = 2.0 ** -24
C = 6.0
SLAB = 512                                          # DLWPCS_ROW_GRAM_SLAB_COLS
GROUP = 16                                          # DLWPCS_ROW_GRAM_GROUP_SLABS
TILE = 128                                          # rows of a tile (the row table brackets it and the 32-row MFMA blocks)
ROWS = [1, 2, 31, 32, 33, 127, 128, 129, 260]
COLUMNS = [1, 31, 33, 511, 512, 513, 8191, 8192, 8193, 16389]
CROSS_TB = [1, 5, 15, 130]
LAYOUTS = ['first', 'middle', 'last', 'sliced', 'offset']
NAN_BITS = (0x7FC00000, 0x7FA00000, 0xFFC00000, 0xFF800001, 0x7F800000, 0xFF800000)       # spectrum_ref.NAN_BITS


def nonfinite(x):
    return (np.asarray(x, dtype=np.float32).view(np.uint32) & 0x7F800000) == 0x7F800000


def n_slabs(E):
    return (E + SLAB - 1) // SLAB


def n_groups(E):
    return (n_slabs(E) + GROUP - 1) // GROUP


def series(rng, T, E, base=280.0, amp=10.0):
    """(T, E) float32 values near `base` with anomalies of order `amp` that are correlated between the rows"""
    common = rng.standard_normal((1, E))
    return (base + amp * (0.6 * common + rng.standard_normal((T, E)))).astype(np.float32)


def own_mean32(x):
    """(E,) float32: the fp64 sum of the rows in row order over the row count, rounded once"""
    s = np.zeros(x.shape[1], dtype=np.float64)
    for t in range(x.shape[0]):
        s = s + x[t].astype(np.float64)
    with np.errstate(all='ignore'):
        return (s / np.float64(max(x.shape[0], 1))).astype(np.float32)


def anomalies(a, b=None, r=None, center_a=True, center_b=None, given_a=None, given_b=None):
    """(y_a, y_b or None, mean of a with NaN at excluded columns, kept): the float32 y of the definition, zero at excluded columns"""
    a = np.asarray(a, dtype=np.float32)
    E = a.shape[1]
    center_b = center_a if center_b is None else center_b
    r32 = np.ones(E, dtype=np.float32) if r is None else np.asarray(r, dtype=np.float32).reshape(E)
    bad = nonfinite(r32)
    ys, means = [], []
    with np.errstate(all='ignore'):
        for x, own, given in ((a, center_a, given_a), (b, center_b, given_b)):
            if x is None:
                ys.append(None)
                continue
            x = np.asarray(x, dtype=np.float32)
            bad = bad | nonfinite(x).any(axis=0)
            if given is not None:
                m = np.asarray(given, dtype=np.float32).reshape(E)
                bad = bad | np.isnan(m)
            elif own:
                m = own_mean32(x)
            else:
                m = np.zeros(E, dtype=np.float32)
            means.append(m)
            d = (x - m[None, :]).astype(np.float32)
            ys.append((r32[None, :] * d).astype(np.float32))
    for y in ys:
        if y is not None:
            y[:, bad] = 0.0
    mean = means[0].copy()
    mean[bad] = np.nan
    return ys[0], ys[1], mean, ~bad


def reference(a, b=None, **kw):
    """dict(G (Ta, Tb) float64, diag_a (Ta,), diag_b (Tb,), n_valid, mean (E,) float32, kept (E,) bool)"""
    ya, yb, mean, kept = anomalies(a, b, **kw)
    ya64 = ya.astype(np.float64)
    yb64 = ya64 if yb is None else yb.astype(np.float64)
    G = np.zeros((ya64.shape[0], yb64.shape[0]))
    for lo in range(0, ya64.shape[1], SLAB):                    # slab by slab: the fp64 sums stay short
        G += ya64[:, lo:lo + SLAB] @ yb64[:, lo:lo + SLAB].T
    return dict(G=G, diag_a=(ya64 ** 2).sum(axis=1), diag_b=(yb64 ** 2).sum(axis=1), n_valid=int(kept.sum()), mean=mean, kept=kept)


def bound(ref):
    return (SLAB + C) * EPS * np.sqrt(np.outer(ref['diag_a'], ref['diag_b']))


def emulate(a, b=None, **kw):
    ya, yb, _, _ = anomalies(a, b, **kw)
    yb = ya if yb is None else yb
    Ta, E = ya.shape
    total = np.zeros((Ta, yb.shape[0]))
    for g in range(n_groups(E)):
        grp = np.zeros_like(total)
        for s in range(g * GROUP, min((g + 1) * GROUP, n_slabs(E))):
            acc = np.zeros(total.shape, dtype=np.float32)
            for q in range(s * SLAB, min((s + 1) * SLAB, E)):
                prod = np.outer(ya[:, q].astype(np.float64), yb[:, q].astype(np.float64))
                acc = (prod + acc.astype(np.float64)).astype(np.float32)
            grp = grp + acc.astype(np.float64)
        total = total + grp
    return total
