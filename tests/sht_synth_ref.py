"""
Bounds, emulation and case tables of the spherical-harmonic analysis / synthesis tests (test_sht_synth_ref.py, test_sht_synth.py,
test_gpu_sht_synth.py).  Not a test module.  Definitions, quadratures and the float64 reference are those of sht_ref.py.

Coefficients travel packed: row spharm.packed_row(m, n, T); pack() / unpack() go between that and sht_ref's dense a[m, n].

analysis_bound(): the device's error in a coefficient, |da_n^m| <= g_a sqrt(M) as a complex number, M the field's quadrature-
  weighted mean square.  sht_ref.bound derives g = (L + nlat + 4) u for the sum before the division; dlwpcs_sht_analysis divides by
  L with one more fp32 rounding, at most u |a_n^m| <= u sqrt(M) (Bessel), so g_a = (L + nlat + 5) u.

synthesis_bound(): the device's error in a grid value, derived for the kernels as written (csrc/sht.hip), u = 2^-24.
  Inverse Legendre: G_m(i) = sum_{n=m..T} P32[(m,n)][i] b_n with b_n = fl(r32_n a_n^m) for Re and for Im: an fp32 dot product of
  at most T + 1 terms whose factors carry three roundings (the table entry, the response r32_n = fl(r_n), the product r a), so
      |dG_m(i)| <= (T + 1 + 3) u sum_n |Pbar_n^m(mu_i)| |r_n| |a_n^m|          (Re with |Re a|, Im with |Im a|; first order).
  Inverse Fourier: x_ij = sum_m (c_m cos) Re G_m + (-c_m sin) Im G_m, an fp32 dot product of 2 (T + 1) terms whose twiddle is
  rounded once (c_m is exact), so its own error is at most (2 (T + 1) + 1) u sum_m c_m (|cos| |Re G_m| + |sin| |Im G_m|), and it
  passes the first stage's error on with the weights c_m |cos|, c_m |sin|.  With |cos| |Re a| + |sin| |Im a| <= |a| (Cauchy-Schwarz)
      |dx_ij| <= k(T) u sum_m c_m sum_n |Pbar_n^m(mu_i)| |r_n a_n^m|,   k(T) = (T + 1) + 2 (T + 1) + 4 + 2 = 3 T + 9:
  the two dot-product lengths, the four roundings, and two u of room for the second-order terms (k u < 7e-5 at T = 360).  Im a_n^0
  does not enter the kernel, so m = 0 counts |Re a_n^0|.  The order of the additions does not enter.

emulate_analysis() / emulate_synthesis(): the kernels' scheme in numpy float32, one rounding per operation, in the kernels' order
  of summation.  They emulate the scheme, not the matrix cores' internal rounding: they show that the bounds hold for a
  sequential fp32 evaluation, without a device.
"""
import numpy as np

import sht_ref as R

EPS = R.EPS
GPU_NLAT = [10, 19, 33, 48]
GPU_L = [12, 37, 72, 96, 100]
WIDE = ('gauss', 132, 264, 131, 2)          # across stage A's 128 orders per workgroup


def packed_rows(T):
    return (T + 1) * (T + 2) // 2


def pack(a):
    """dense a[..., m, n] -> packed (..., rows)"""
    T = a.shape[-1] - 1
    return np.concatenate([a[..., m, m:] for m in range(T + 1)], axis=-1)


def unpack(c, T):
    """packed (..., rows) -> dense a[..., m, n], zero for n < m"""
    a = np.zeros(c.shape[:-1] + (T + 1, T + 1), dtype=c.dtype)
    at = 0
    for m in range(T + 1):
        a[..., m, m:] = c[..., at:at + T + 1 - m]
        at += T + 1 - m
    return a


def grid_cases():
    """[(kind, nlat, L, T, fields, south_first)]: the nlat x L grid with the quadratures, the field counts and the latitude
    direction rotating through it, every shape at the largest T it allows and at T = 0; the truncations on and across the
    32-degree tile at gauss 48 x 96; the case across stage A's 128 orders"""
    out = []
    i = 0
    for nlat in GPU_NLAT:
        for L in GPU_L:
            kind = R.KINDS[i % 3]
            for T in sorted(set((R.max_truncation(kind, nlat, L), 0))):
                out.append((kind, nlat, L, T, R.GPU_FIELDS[(i // 2) % 5], bool((i // 3) % 2)))
                i += 1
    out += [('gauss', 48, 96, T, 3, False) for T in R.GPU_T_EDGE]
    out.append(WIDE + (False,))
    return out


# ---- float64 references ---------------------------------------------------------------------------------------------- #

def analysis(x, kind, T):
    """packed complex coefficients (..., rows) of fields x (..., nlat, L), north to south"""
    return pack(R.analysis(x, R.table(kind, x.shape[-2], T)))


def synthesis(c, kind, nlat, L, response=None):
    """fields (..., nlat, L) of packed coefficients c (..., rows); Im a_n^0 is ignored.  Written on its own: dense P[m, n, i], an
    explicit sum over m with cos and sin."""
    rows = c.shape[-1]
    T = int(round((np.sqrt(8.0 * rows + 1.0) - 3.0) / 2.0))
    a = unpack(np.asarray(c, dtype=np.complex128), T)
    if response is not None:
        a = a * np.asarray(response, dtype=np.float64)
    P = R.pbar(R.sin_lat(kind, nlat), T)
    G = np.einsum('...mn,mni->...mi', a, P)
    lon = 2 * np.pi * np.arange(L) / L
    cm = R.c_m(T)
    x = np.zeros(c.shape[:-1] + (nlat, L))
    for m in range(T + 1):
        re, im = G[..., m, :].real, (G[..., m, :].imag if m else 0.0 * G[..., m, :].real)
        x += cm[m] * (re[..., None] * np.cos(m * lon) - im[..., None] * np.sin(m * lon))
    return x


def random_packed(rng, T, shape=(), slope=0.0):
    """packed coefficients (shape..., rows), real for m = 0, amplitude (n + 1)^-slope"""
    a = np.array([R.random_coefficients(rng, T, slope) for _ in range(int(np.prod(shape, dtype=np.int64)))])
    return pack(a).reshape(tuple(shape) + (packed_rows(T),))


# ---- bounds ---------------------------------------------------------------------------------------------------------- #

def analysis_bound(x, kind):
    """the largest allowed |device - reference| of any coefficient of the fields x (..., nlat, L): (...,)"""
    nlat, L = x.shape[-2:]
    return (L + nlat + 5) * EPS * np.sqrt(R.mean_square(x, kind))


def k_synthesis(T):
    return 3 * T + 9


def synthesis_bound(c, kind, nlat, response=None):
    """the largest allowed |device - reference| (..., nlat) of the grid values of a latitude, for packed coefficients c (..., rows)
    in the values the device was given"""
    rows = c.shape[-1]
    T = int(round((np.sqrt(8.0 * rows + 1.0) - 3.0) / 2.0))
    a = unpack(np.asarray(c, dtype=np.complex128), T)
    mag = np.abs(a)
    mag[..., 0, :] = np.abs(a[..., 0, :].real)
    if response is not None:
        mag = mag * np.abs(np.asarray(response, dtype=np.float64))
    P = np.abs(R.pbar(R.sin_lat(kind, nlat), T))
    s = np.einsum('m,...mn,mni->...i', R.c_m(T), mag, P)
    return k_synthesis(T) * EPS * s


# ---- the schemes of the kernels in sequential fp32 ----------------------------------------------------------------- #

def emulate_analysis(x, kind, T):
    """packed complex64 coefficients of fields x (F, nlat, L): stage A and stage B as sht_ref.emulate orders them, then the
    division by L rounded once"""
    f32 = np.float32
    x = np.asarray(x, dtype=f32)
    F, nlat, L = x.shape
    ang = 2.0 * np.pi * np.arange(L) / L
    tw = np.stack([np.cos(ang), -np.sin(ang)], axis=1).astype(f32)
    t32 = R.table(kind, nlat, T).astype(f32)
    order_j = [4 * s + u for s in range((L + 3) // 4) for u in (0, 2, 1, 3) if 4 * s + u < L]
    order_i = [32 * s + u + k for s in range((nlat + 31) // 32) for u in range(16) for k in (0, 16) if 32 * s + u + k < nlat]
    m = np.arange(T + 1)
    X = np.zeros((2, F, nlat, T + 1), dtype=f32)
    for j in order_j:
        twj = tw[(j * m) % L]
        for c in range(2):
            X[c] = (X[c] + (x[:, :, j, None] * twj[None, None, :, c]).astype(f32)).astype(f32)
    a = np.zeros((2, F, T + 1, T + 1), dtype=f32)
    for i in order_i:
        for c in range(2):
            a[c] = (a[c] + (t32[None, :, :, i] * X[c][:, i, :, None]).astype(f32)).astype(f32)
    a = (a.astype(np.float64) / float(L)).astype(f32)
    return pack(a[0] + 1j * a[1]).astype(np.complex64)


def emulate_synthesis(c, kind, nlat, L, response=None):
    """float32 fields (F, nlat, L) of packed complex64 coefficients c (F, rows): the inverse Legendre stage in order of n, the
    inverse Fourier stage in order of m (Re before Im), every product and sum rounded to fp32"""
    f32 = np.float32
    rows = c.shape[-1]
    T = int(round((np.sqrt(8.0 * rows + 1.0) - 3.0) / 2.0))
    a = unpack(np.asarray(c, dtype=np.complex64), T)
    r = np.ones(T + 1, dtype=f32) if response is None else np.asarray(response, dtype=np.float64).astype(f32)
    b = np.stack([(a.real.astype(f32) * r).astype(f32), (a.imag.astype(f32) * r).astype(f32)])       # [re | im, F, m, n]
    b[1][:, 0, :] = 0.0
    P32 = R.pbar(R.sin_lat(kind, nlat), T).astype(f32)                                                # [m, n, i]
    F = a.shape[0]
    G = np.zeros((2, F, T + 1, nlat), dtype=f32)
    for n in range(T + 1):
        for q in range(2):
            G[q] = (G[q] + (P32[None, :, n, :] * b[q][:, :, n, None]).astype(f32)).astype(f32)
    ang = 2.0 * np.pi * np.arange(L) / L
    tw = np.stack([np.cos(ang), -np.sin(ang)], axis=1).astype(f32)
    j = np.arange(L)
    x = np.zeros((F, nlat, L), dtype=f32)
    for m in range(T + 1):
        cm = f32(1.0 if m == 0 else 2.0)
        t = tw[(j * m) % L]
        for q in range(2):
            x = (x + (G[q][:, m, :, None] * (cm * t[None, None, :, q])).astype(f32)).astype(f32)
    return x
