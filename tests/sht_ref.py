"""
Reference, bound, emulation and case tables of the spherical-harmonic spectrum tests (test_sht_ref.py, test_sht.py,
test_gpu_sht.py).  Not a test module.

Definitions (include/dlwpcs.h, DLWP/remap/spharm.py): a field x[i, j] on nlat latitudes (mu_i = sin lat_i, weights w_i >= 0,
sum w_i = 2) and L equally spaced longitudes; Pbar_n^m with (1/2) int Pbar_n^m Pbar_n'^m dmu = delta_nn';
    X_m(i) = sum_j x[i,j] exp(-2 pi i j m / L),  a_n^m = sum_i (w_i / 2) Pbar_n^m(mu_i) X_m(i) / L,  S_n = sum_{m<=n} c_m |a_n^m|^2.
Everything here is float64 and written on its own: the recurrence, the three weight formulas, the analysis as one einsum per
call over a dense (m, n, i) array, and a synthesis that only makes band-limited inputs.

bound(): the device's error, derived for the kernel as it is written (csrc/sht.hip), u = 2^-24.
  Stage A is an fp32 dot product of length L with twiddles rounded once: per row |dX_m(i)| <= (L + 1) u sum_j |x_ij| |tw_j|
  for Re and for Im, hence (Cauchy-Schwarz over j, cos^2 + sin^2 = 1) |dX_m(i)| / L <= (L + 1) u r_i as a complex number, with
  r_i^2 = mean_j x_ij^2.  Stage B is an fp32 dot product of length nlat with a table rounded once: its own error is at most
  (nlat + 1) u sum_i |t_i| |X_m(i)| / L <= (nlat + 1) u sum_i |t_i| r_i, again for the complex number (Minkowski over i).  With
  t_i = (w_i / 2) Pbar_n^m(mu_i), w_i >= 0 and the table's orthonormality, sum_i |t_i| r_i <= sqrt(sum_i (w_i/2) Pbar^2)
  sqrt(sum_i (w_i/2) r_i^2) = sqrt(M), M the field's quadrature-weighted mean square.  So |da_n^m| <= g sqrt(M) with
  g = (L + nlat + 4) u (two u of room for the second-order terms; the order of the additions does not enter).
  S_n: sum_m c_m (2 |a| |da| + |da|^2) <= E = 2 g sqrt((2n + 1) ref_n M) + g^2 (2n + 1) M (Cauchy-Schwarz over m, sum_m c_m =
  2n + 1).  The fp32 product Re^2 + Im^2 (one multiply, one fma) adds 2 u of the computed term, the final rounding 1 u:
      |S_n - ref_n| <= E + 4 u (ref_n + E).
  Co-spectrum: E_c = g sqrt(2n + 1) (sqrt(ref_ff M_v) + sqrt(ref_vv M_f)) + g^2 (2n + 1) sqrt(M_f M_v), and
      |C_n - ref_n| <= E_c + 4 u (sqrt(ref_ff ref_vv) + E_c).
  A mean over G fields (dlwpcs_group_mean: fp64 sum of the fp32 rows, one rounding at the end): the mean of the fields' bounds
  (each holds its row's rounding already) plus u (|mean ref| + mean bound) for the last rounding.
"""
import numpy as np

EPS = 2.0 ** -24
KINDS = ('clenshaw-curtis', 'fejer', 'gauss')
NAN_BITS = (0x7FC00000, 0x7FA00000, 0xFFC00000, 0xFF800001, 0x7F800000, 0xFF800000)       # NaN payloads and +-inf

GPU_NLAT = [2, 5, 17, 33, 64, 65]
GPU_L = [8, 12, 37, 72, 130]
GPU_FIELDS = [1, 3, 32, 33, 70]
GPU_T_EDGE = [31, 32, 33, 40]               # at gauss nlat = 48, L = 96
# the five cases of the sequential-fp32 emulation: (kind, nlat, L, T)
EMULATED = [('clenshaw-curtis', 17, 32, 8), ('clenshaw-curtis', 33, 64, 16), ('fejer', 16, 36, 7), ('gauss', 24, 50, 23),
            ('clenshaw-curtis', 91, 180, 45)]


# ---- quadratures ----------------------------------------------------------------------------------------------------- #

def colatitudes(kind, nlat):
    """radians, north to south"""
    if kind == 'gauss':
        return np.arccos(-np.polynomial.legendre.leggauss(nlat)[0])
    if kind == 'clenshaw-curtis':
        return np.arange(nlat) * np.pi / (nlat - 1)
    return (2 * np.arange(nlat) + 1) * np.pi / (2 * nlat)


def latitudes(kind, nlat, south_first=False):
    """degrees"""
    lat = 90.0 - np.degrees(colatitudes(kind, nlat))
    return lat[::-1].copy() if south_first else lat


def sin_lat(kind, nlat):
    if kind == 'gauss':
        return -np.polynomial.legendre.leggauss(nlat)[0]
    mu = np.cos(colatitudes(kind, nlat))
    if kind == 'clenshaw-curtis':
        mu[0], mu[-1] = 1.0, -1.0
    return mu


def weights(kind, nlat):
    """the formulas of DESIGN.md 4.18, term by term with plain loops"""
    if kind == 'gauss':
        return np.polynomial.legendre.leggauss(nlat)[1][::-1].copy()
    th = colatitudes(kind, nlat)
    w = np.empty(nlat)
    if kind == 'clenshaw-curtis':
        N = nlat - 1
        for i in range(nlat):
            s = sum((1.0 if 2 * k == N else 2.0) * np.cos(2 * k * th[i]) / (4 * k * k - 1) for k in range(1, N // 2 + 1))
            w[i] = (1.0 if i in (0, N) else 2.0) / N * (1.0 - s)
        return w
    for i in range(nlat):
        s = sum(np.cos(2 * k * th[i]) / (4 * k * k - 1) for k in range(1, nlat // 2 + 1))
        w[i] = 2.0 / nlat * (1.0 - 2.0 * s)
    return w


def exact_degree(kind, nlat):
    """the largest polynomial degree the rule integrates exactly"""
    if kind == 'gauss':
        return 2 * nlat - 1
    return nlat - 1 if nlat % 2 == 0 else nlat          # interpolatory on nlat nodes; symmetric rules gain one odd degree


def max_truncation(kind, nlat, L):
    return max(min(nlat - 1 if kind == 'gauss' else (nlat - 1) // 2, (L - 1) // 2), 0)


# ---- Legendre functions ---------------------------------------------------------------------------------------------- #

def pbar(mu, T):
    """P[m, n, i] = Pbar_n^m(mu_i), zero for n < m"""
    mu = np.asarray(mu, dtype=np.float64)
    c = np.sqrt(np.maximum(1.0 - mu * mu, 0.0))
    P = np.zeros((T + 1, T + 1, mu.size))
    for m in range(T + 1):
        P[m, m] = 1.0 if m == 0 else np.sqrt((2 * m + 1) / (2 * m)) * c * P[m - 1, m - 1]
        if m + 1 <= T:
            P[m, m + 1] = np.sqrt(2 * m + 3) * mu * P[m, m]
        for n in range(m + 2, T + 1):
            A = np.sqrt((4 * n * n - 1) / (n * n - m * m))
            B = np.sqrt(((n - 1) ** 2 - m * m) / (4 * (n - 1) ** 2 - 1))
            P[m, n] = A * (mu * P[m, n - 1] - B * P[m, n - 2])
    return P


def table(kind, nlat, T):
    """t[m, n, i] = (w_i / 2) Pbar_n^m(mu_i), north to south"""
    return pbar(sin_lat(kind, nlat), T) * (0.5 * weights(kind, nlat))


def packed_rows_brute(T):
    """[(m, n)] in the order of the packed table"""
    return [(m, n) for m in range(T + 1) for n in range(m, T + 1)]


def c_m(T):
    c = np.full(T + 1, 2.0)
    c[0] = 1.0
    return c


# ---- analysis and synthesis ------------------------------------------------------------------------------------------ #

def analysis(x, t):
    """a[..., m, n] complex for fields x (..., nlat, L) and the table t[m, n, i]"""
    x = np.asarray(x, dtype=np.float64)
    T = t.shape[0] - 1
    X = np.fft.rfft(x, axis=-1)[..., :T + 1] / x.shape[-1]
    return np.einsum('mni,...im->...mn', t, X)


def synthesis(a, kind, nlat, L):
    """x[i, j] = sum_{n, m} c_m Re(a[m, n] Pbar_n^m(mu_i) exp(i m lon_j)); a[0, n] must be real.  Only makes test inputs."""
    T = a.shape[0] - 1
    P = pbar(sin_lat(kind, nlat), T)
    lon = 2 * np.pi * np.arange(L) / L
    x = np.zeros((nlat, L))
    for m in range(T + 1):
        col = np.einsum('n,ni->i', a[m], P[m])                      # (nlat,) complex
        x += c_m(T)[m] * (col[:, None] * np.exp(1j * m * lon)[None, :]).real
    return x


def random_coefficients(rng, T, slope=0.0):
    """a[m, n] for n >= m, real for m = 0, amplitude (n + 1)^-slope"""
    a = (rng.standard_normal((T + 1, T + 1)) + 1j * rng.standard_normal((T + 1, T + 1))) * np.triu(np.ones((T + 1, T + 1)))
    a[0] = a[0].real
    return a * (np.arange(T + 1) + 1.0)[None, :] ** -slope


def power(af, av=None):
    """(nq, ..., T + 1): S_ff (, S_vv, co) from coefficients a[..., m, n]"""
    T = af.shape[-1] - 1
    c = c_m(T)[:, None]
    q = [(c * np.abs(af) ** 2).sum(axis=-2)]
    if av is not None:
        q += [(c * np.abs(av) ** 2).sum(axis=-2), (c * (af * np.conj(av)).real).sum(axis=-2)]
    return np.array(q)


def mean_square(x, kind):
    """M: the quadrature-weighted mean square of fields x (..., nlat, L)"""
    x = np.asarray(x, dtype=np.float64)
    return np.einsum('i,...i->...', 0.5 * weights(kind, x.shape[-2]), (x * x).mean(axis=-1))


def bound(nlat, L, ref, M):
    """ref (nq, ..., K) and M (2, ...) of single fields -> the largest allowed |device - reference| (nq, ..., K)"""
    g = (L + nlat + 4) * EPS
    K = ref.shape[-1]
    d = 2.0 * np.arange(K) + 1.0
    Mf, Mv = M[0][..., None], M[1][..., None]
    r0 = np.maximum(ref[0], 0.0)
    E = 2 * g * np.sqrt(d * r0 * Mf) + g * g * d * Mf
    out = [E + 4 * EPS * (r0 + E)]
    if ref.shape[0] > 1:
        r1 = np.maximum(ref[1], 0.0)
        E1 = 2 * g * np.sqrt(d * r1 * Mv) + g * g * d * Mv
        Ec = g * np.sqrt(d) * (np.sqrt(r0 * Mv) + np.sqrt(r1 * Mf)) + g * g * d * np.sqrt(Mf * Mv)
        out += [E1 + 4 * EPS * (r1 + E1), Ec + 4 * EPS * (np.sqrt(r0 * r1) + Ec)]
    return np.array(out)


def reference(f, v, kind, T, axis=(), south_first=False):
    """
    f, v: arrays (..., nlat, L) (v None: single form); axis: the averaged leading axes.
    Returns (out (nq, kept..., K) float64, skipped (kept...) int64, lim (nq, kept..., K): the bound of every result).
    """
    pair = v is not None
    with np.errstate(invalid='ignore'):                             # (signalling NaN payloads among the test inputs)
        f = np.asarray(f, dtype=np.float64)
        v = np.asarray(v, dtype=np.float64) if pair else f
    nlat, L = f.shape[-2:]
    lead = f.shape[:-2]
    axis = tuple(sorted(a % len(lead) for a in axis)) if lead else ()
    kept = [i for i in range(len(lead)) if i not in axis]
    perm = kept + list(axis)
    n_groups = int(np.prod([lead[i] for i in kept], dtype=np.int64))
    fr = f.transpose(perm + [len(lead), len(lead) + 1]).reshape(n_groups, -1, nlat, L)
    vr = v.transpose(perm + [len(lead), len(lead) + 1]).reshape(n_groups, -1, nlat, L)
    if south_first:
        fr, vr = fr[:, :, ::-1], vr[:, :, ::-1]
    t = table(kind, nlat, T)
    nq = 3 if pair else 1
    out = np.full((nq, n_groups, T + 1), np.nan)
    lim = np.full((nq, n_groups, T + 1), np.nan)
    skipped = np.zeros(n_groups, dtype=np.int64)
    for g in range(n_groups):
        ok = np.isfinite(fr[g]).all(axis=(-2, -1)) & np.isfinite(vr[g]).all(axis=(-2, -1))
        skipped[g] = (~ok).sum()
        if not ok.any():
            continue
        x, y = fr[g][ok], vr[g][ok]
        q = power(analysis(x, t), analysis(y, t) if pair else None)             # (nq, G, K)
        b = bound(nlat, L, q, np.array([mean_square(x, kind), mean_square(y, kind)]))
        out[:, g] = q.mean(axis=1)
        lim[:, g] = b.mean(axis=1)
        if x.shape[0] > 1:
            lim[:, g] += EPS * (np.abs(out[:, g]) + lim[:, g])
    shape = tuple(lead[i] for i in kept)
    return out.reshape((nq,) + shape + (T + 1,)), skipped.reshape(shape), lim.reshape((nq,) + shape + (T + 1,))


# ---- the scheme of the kernel in sequential fp32 ------------------------------------------------------------------- #

def emulate(f, v, kind, T):
    """the device's scheme on fields (F, nlat, L) in numpy float32, one rounding per operation: stage A in the order of the
    kernel's longitude steps, stage B in the order of its latitude steps, the fp32 products, the fp64 sum over m.  It is an
    emulation of the scheme, not of the matrix cores' internal rounding: it shows the bound holds, not the bits."""
    f32 = np.float32
    ops = [np.asarray(f, dtype=f32)] + ([np.asarray(v, dtype=f32)] if v is not None else [])
    F, nlat, L = ops[0].shape
    ang = 2.0 * np.pi * np.arange(L) / L
    tw = np.stack([np.cos(ang), -np.sin(ang)], axis=1).astype(f32)
    t32 = table(kind, nlat, T).astype(f32)
    order_j = [4 * s + u for s in range((L + 3) // 4) for u in (0, 2, 1, 3) if 4 * s + u < L]
    order_i = [32 * s + u + k for s in range((nlat + 31) // 32) for u in range(16) for k in (0, 16) if 32 * s + u + k < nlat]
    m = np.arange(T + 1)
    coef = []
    for x in ops:
        X = np.zeros((2, F, nlat, T + 1), dtype=f32)
        for j in order_j:
            twj = tw[(j * m) % L]                                               # (T + 1, 2)
            for c in range(2):
                X[c] = (X[c] + (x[:, :, j, None] * twj[None, None, :, c]).astype(f32)).astype(f32)
        a = np.zeros((2, F, T + 1, T + 1), dtype=f32)                           # [re | im, field, m, n]
        for i in order_i:
            for c in range(2):
                a[c] = (a[c] + (t32[None, :, :, i] * X[c][:, i, :, None]).astype(f32)).astype(f32)
        coef.append(a)
    af, av = coef[0], coef[-1]

    def prod(p, q):
        return ((p[1] * q[1]).astype(f32) + (p[0] * q[0]).astype(f32)).astype(f32)
    prods = [prod(af, af)] + ([prod(av, av), prod(af, av)] if v is not None else [])
    scale = c_m(T) / float(L) ** 2
    out = []
    for p in prods:
        s = np.zeros((F, T + 1))
        for mm in range(T + 1):
            s += p[:, mm, :].astype(np.float64) * scale[mm]
        out.append(s.astype(f32))
    return np.array(out)


# ---- inputs ---------------------------------------------------------------------------------------------------------- #

def make_field(rng, shape, kind='white', offset=0.0):
    """float32 test fields (..., nlat, L): white noise, red noise (a random walk along longitude, then latitude) or noise on an
    offset.  They are NOT band-limited: the device and the reference analyse the same grid values."""
    x = rng.standard_normal(shape)
    if kind == 'red':
        x = np.cumsum(np.cumsum(x, axis=-1), axis=-2) / 8.0
    return (x + offset).astype(np.float32)


def grid_cases():
    """[(kind, nlat, L, T, fields, pair)]: the nlat x L grid, the quadratures, the field counts and the two forms rotating
    through it; every shape at the largest T it allows and at T = 0"""
    out = []
    i = 0
    for nlat in GPU_NLAT:
        for L in GPU_L:
            kind = KINDS[i % 3]
            for T in sorted(set((max_truncation(kind, nlat, L), 0))):
                out.append((kind, nlat, L, T, GPU_FIELDS[(i // 2) % 5], bool(i % 2)))
                i += 1
    return out


def groups_reference(lead, red):
    """what ops.sht_groups_host must produce, by brute force: [[field numbers of group g in order]]"""
    lead = tuple(lead)
    kept = [i for i in range(len(lead)) if i not in red]
    groups = {}
    for flat, idx in enumerate(np.ndindex(*lead)):
        groups.setdefault(tuple(idx[i] for i in kept), []).append(flat)
    return [groups[k] for k in sorted(groups)]
