"""
Bounds, emulation and case tables of the vector spherical-harmonic and barotropic-model tests (test_sht_vector_ref.py,
test_sht_vector.py, test_barotropic.py, test_gpu_sht_vector.py, test_gpu_barotropic.py).  Not a test module.  Quadratures and
Legendre functions are those of sht_ref.py, the packing that of sht_synth_ref.py.

dense_tables(): D[m, n, i] = dPbar_n^m / dphi and Q[m, n, i] = m Pbar_n^m / cos(phi) from sht_ref.pbar, written on their own (the
  pole rows by the limit formula); everything below works north to south.

synthesis_bound(): the device's error in a grid value of u and of v, derived for the kernels as written (csrc/sht.hip), u = 2^-24.
  Inverse vector Legendre: Re U_m(i) = sum_n D (-psi_re) + Q (-chi_im) and its three siblings are fp32 dot products of at most
  p (T + 1) terms (p potentials present) whose factors carry three roundings (table entry, response, product r a):
      |d Re U_m(i)| <= (p (T + 1) + 3) u sum_n (|D| |psi_re| + |Q| |chi_im|),   and alike with (psi_im, chi_re) for Im U_m.
  Inverse Fourier as in sht_synth_ref: 2 (T + 1) terms, one rounding of the twiddle, and |cos| |x_re| + |sin| |x_im| <= |x|:
      |du_ij| <= k u sum_m c_m sum_n (|D_n^m(mu_i)| |rpsi_n A_n^m| + |Q_n^m(mu_i)| |rchi_n B_n^m|),   k = (p + 2)(T + 1) + 6,
      |dv_ij| <= k u sum_m c_m sum_n (|Q_n^m(mu_i)| |rpsi_n A_n^m| + |D_n^m(mu_i)| |rchi_n B_n^m|)
  (two u of room for the second-order terms, as there).  Im of order 0 does not enter the kernel: m = 0 counts |Re|.

analysis_bound(): the device's error in Re and in Im of a coefficient.  Stage A: Re and Im of X_m(i) are fp32 dot products of L
  terms with a twiddle rounded once: at most (L + 1) u S(i), S(i) = sum_j |x_ij|.  The coefficient stage: a dot product of 2 nlat
  terms with table entries rounded once, (2 nlat + 1) u sum_i (|wD| |U_m| + |wQ| |V_m|), |X_m(i)| <= S(i), and it passes stage
  A's error on with the weights |wD|, |wQ|.  The response is rounded once and the result once (the fp64 steps in between add
  2^-52): with two u of room
      |d Re vrt_n^m|, |d Im vrt_n^m| <= (L + 2 nlat + 6) u |r_n| sum_i (|wD_n^m(i)| S_u(i) + |wQ_n^m(i)| S_v(i)) / L
      |d Re div_n^m|, |d Im div_n^m| <= (L + 2 nlat + 6) u |r_n| sum_i (|wQ_n^m(i)| S_u(i) + |wD_n^m(i)| S_v(i)) / L.

analysis_propagation() / scalar_analysis_propagation(): how an exact analysis passes on the error bound of the grid it is given, so
  that the bounds of the links of a chain (synthesis, then analysis) add up to a bound of the chain.

emulate_synthesis() / emulate_analysis(): the kernels' scheme in numpy float32, one rounding per operation, in the kernels' order
  of summation (pairs of degrees: psi before chi; pairs of latitudes i, i + 16: vrt takes wD before wQ, div wQ before wD).  They
  emulate the scheme, not the matrix cores' internal rounding.  emulate_model() steps the barotropic model with them and the
  update kernel's operations spelled in float32: its distance from the float64 twin, times 4, is the allowance of the device
  model (test_gpu_barotropic.py): the factor allows for the device's different but fixed summation order.
"""
import numpy as np

import sht_ref as R
import sht_synth_ref as S

EPS = R.EPS
f32 = np.float32

# (kind, nlat, L): the round trip runs at the scalar transform's own largest truncation
ROUND_TRIP = [('gauss', 8, 16), ('gauss', 33, 66), ('fejer', 16, 32), ('fejer', 33, 64), ('fejer', 90, 180),
              ('clenshaw-curtis', 9, 16), ('clenshaw-curtis', 17, 32), ('clenshaw-curtis', 33, 64), ('clenshaw-curtis', 181, 360)]

WIDE = ('gauss', 132, 264, 131, 2, False)       # across stage A's 128 orders per workgroup

# (kind, nlat, L, T, fields, south_first): nlat in {2, 10, 19, 33, 48} (19: the padding to 4; 33: across the latitude tile),
# L in {12, 37, 72, 100} (odd, no multiple of 4, the element path), T in {0, 1, 31, 32, 33, the largest}, fields in {1, 32, 33, 65}
GPU_CASES = [('gauss', 2, 12, 1, 1, False), ('gauss', 2, 12, 0, 33, True),
             ('clenshaw-curtis', 10, 37, 4, 32, False), ('fejer', 10, 12, 4, 65, True),
             ('clenshaw-curtis', 19, 37, 9, 33, True), ('fejer', 19, 72, 9, 1, False), ('gauss', 19, 100, 18, 32, False),
             ('gauss', 33, 72, 32, 33, False), ('clenshaw-curtis', 33, 100, 16, 65, False), ('gauss', 33, 100, 1, 3, False),
             ('gauss', 48, 72, 31, 3, True), ('gauss', 48, 100, 33, 3, False), ('gauss', 48, 100, 47, 32, False),
             ('fejer', 48, 37, 18, 33, False), WIDE]


def dense_tables(kind, nlat, T):
    """(D, Q), each [m, n, i] north to south, zero for n < m"""
    mu = R.sin_lat(kind, nlat)
    P = R.pbar(mu, T + 1)
    cos_lat = np.sqrt(np.maximum(1.0 - mu * mu, 0.0))
    pole = cos_lat == 0.0
    ic = 1.0 / np.where(pole, 1.0, cos_lat)
    D, Q = np.zeros((T + 1, T + 1, nlat)), np.zeros((T + 1, T + 1, nlat))
    eps = lambda n, m: np.sqrt((n * n - m * m) / (4.0 * n * n - 1.0))          # noqa: E731
    for m in range(T + 1):
        for n in range(m, T + 1):
            d = -n * eps(n + 1, m) * P[m, n + 1]
            if n > m:
                d = d + (n + 1) * eps(n, m) * P[m, n - 1]
            D[m, n] = d * ic
            Q[m, n] = m * P[m, n] * ic
    if pole.any():
        D[:, :, pole], Q[:, :, pole] = 0.0, 0.0
        x = mu[pole]
        p = np.zeros((T + 2, x.size))
        if T >= 1:
            p[1] = np.sqrt(1.5)
        for n in range(2, T + 1):
            A = np.sqrt((4.0 * n * n - 1.0) / (n * n - 1.0))
            B = np.sqrt(((n - 1.0) ** 2 - 1.0) / (4.0 * (n - 1.0) ** 2 - 1.0))
            p[n] = A * (x * p[n - 1] - B * p[n - 2])
        for n in range(1, T + 1):
            Q[1, n][pole] = p[n]
            D[1, n][pole] = -x * p[n]
    return D, Q


def _mag(c, T, response):
    a = S.unpack(np.asarray(c, dtype=np.complex128), T)
    mag = np.abs(a)
    mag[..., 0, :] = np.abs(a[..., 0, :].real)
    if response is not None:
        mag = mag * np.abs(np.asarray(response, dtype=np.float64))
    return mag


def k_synthesis(T, potentials):
    return (potentials + 2) * (T + 1) + 6


def synthesis_bound(A, B, rpsi, rchi, kind, nlat, T):
    """(bound of u, bound of v), each (..., nlat) north to south, for packed coefficients in the values the device was given"""
    D, Q = (np.abs(t) for t in dense_tables(kind, nlat, T))
    su = sv = 0.0
    for c, r, tu, tv in ((A, rpsi, D, Q), (B, rchi, Q, D)):
        if c is None:
            continue
        mag = _mag(c, T, r)
        su = su + np.einsum('m,...mn,mni->...i', R.c_m(T), mag, tu)
        sv = sv + np.einsum('m,...mn,mni->...i', R.c_m(T), mag, tv)
    k = k_synthesis(T, (A is not None) + (B is not None))
    return k * EPS * su, k * EPS * sv


def analysis_bound(u, v, response, kind, T):
    """(bound of vrt, bound of div), each packed (..., rows): the largest allowed |device - reference| of Re and of Im, for fields
    u, v (..., nlat, L) north to south"""
    nlat, L = u.shape[-2:]
    D, Q = (np.abs(t) * (0.5 * R.weights(kind, nlat)) for t in dense_tables(kind, nlat, T))
    Su, Sv = np.abs(u).sum(axis=-1), np.abs(v).sum(axis=-1)
    r = np.ones(T + 1) if response is None else np.abs(np.asarray(response, dtype=np.float64))
    k = (L + 2 * nlat + 6) * EPS / L
    bz = k * r * (np.einsum('mni,...i->...mn', D, Su) + np.einsum('mni,...i->...mn', Q, Sv))
    bd = k * r * (np.einsum('mni,...i->...mn', Q, Su) + np.einsum('mni,...i->...mn', D, Sv))
    return S.pack(bz), S.pack(bd)


def analysis_propagation(bu, bv, response, kind, T):
    """What the EXACT vector analysis makes of grid errors |du_ij| <= bu[..., i], |dv_ij| <= bv[..., i] (per latitude, north to
    south): (bound of vrt, bound of div), packed, on Re and on Im each.  Re and Im of the longitude transform of an error row are
    at most L b_i, the division by L takes the L back: |r_n| sum_i (|wD| bu_i + |wQ| bv_i) for vrt, wD and wQ swapped for div."""
    nlat = bu.shape[-1]
    D, Q = (np.abs(t) * (0.5 * R.weights(kind, nlat)) for t in dense_tables(kind, nlat, T))
    r = np.ones(T + 1) if response is None else np.abs(np.asarray(response, dtype=np.float64))
    bz = r * (np.einsum('mni,...i->...mn', D, bu) + np.einsum('mni,...i->...mn', Q, bv))
    bd = r * (np.einsum('mni,...i->...mn', Q, bu) + np.einsum('mni,...i->...mn', D, bv))
    return S.pack(bz), S.pack(bd)


def scalar_analysis_propagation(b, kind, T):
    """the same for the scalar analysis: sum_i (w_i / 2) |Pbar_n^m(mu_i)| b_i, packed, on Re and on Im each"""
    return S.pack(np.einsum('mni,...i->...mn', np.abs(R.table(kind, b.shape[-1], T)), b))


# ---- float64 references, written on their own (dense tables, explicit sums over the orders) -------------------------------- #

def synthesis(A, B, rpsi, rchi, kind, nlat, L, T):
    D, Q = dense_tables(kind, nlat, T)
    lead = (A if A is not None else B).shape[:-1]
    U = np.zeros(lead + (T + 1, nlat), dtype=np.complex128)
    V = np.zeros_like(U)
    for c, r, psi in ((A, rpsi, True), (B, rchi, False)):
        if c is None:
            continue
        a = S.unpack(np.asarray(c, dtype=np.complex128), T)
        a[..., 0, :] = a[..., 0, :].real
        if r is not None:
            a = a * np.asarray(r, dtype=np.float64)
        d, q = np.einsum('...mn,mni->...mi', a, D), np.einsum('...mn,mni->...mi', a, Q)
        if psi:
            U, V = U - d, V + 1j * q
        else:
            U, V = U + 1j * q, V + d
    lon = 2 * np.pi * np.arange(L) / L
    out = []
    for G in (U, V):
        x = np.zeros(lead + (nlat, L))
        for m in range(T + 1):
            x += R.c_m(T)[m] * (G[..., m, :, None] * np.exp(1j * m * lon)).real
        out.append(x)
    return out


def analysis(u, v, response, kind, T):
    nlat, L = u.shape[-2:]
    D, Q = (t * (0.5 * R.weights(kind, nlat)) for t in dense_tables(kind, nlat, T))
    U = np.fft.rfft(np.asarray(u, dtype=np.float64), axis=-1)[..., :T + 1] / L
    V = np.fft.rfft(np.asarray(v, dtype=np.float64), axis=-1)[..., :T + 1] / L
    r = np.ones(T + 1) if response is None else np.asarray(response, dtype=np.float64)
    z = r * (1j * np.einsum('mni,...im->...mn', Q, V) + np.einsum('mni,...im->...mn', D, U))
    d = r * (1j * np.einsum('mni,...im->...mn', Q, U) - np.einsum('mni,...im->...mn', D, V))
    return S.pack(z), S.pack(d)


# ---- the schemes of the kernels in sequential fp32 ----------------------------------------------------------------------- #

def _twiddle(L):
    ang = 2.0 * np.pi * np.arange(L) / L
    return np.stack([np.cos(ang), -np.sin(ang)], axis=1).astype(f32)


def _fourier(x, T):
    """stage A: X[re | im, F, nlat, m] of float32 fields x (F, nlat, L), in the order of sht_synth_ref.emulate_analysis"""
    F, nlat, L = x.shape
    tw = _twiddle(L)
    order_j = [4 * s + u for s in range((L + 3) // 4) for u in (0, 2, 1, 3) if 4 * s + u < L]
    m = np.arange(T + 1)
    X = np.zeros((2, F, nlat, T + 1), dtype=f32)
    for j in order_j:
        twj = tw[(j * m) % L]
        for c in range(2):
            X[c] = (X[c] + (x[:, :, j, None] * twj[None, None, :, c]).astype(f32)).astype(f32)
    return X


def _ifourier(G, L):
    """the inverse Fourier stage: fields (F, nlat, L) of G[re | im, F, m, nlat], in order of m, Re before Im"""
    F, K, nlat = G.shape[1:]
    tw = _twiddle(L)
    j = np.arange(L)
    x = np.zeros((F, nlat, L), dtype=f32)
    for m in range(K):
        cm = f32(1.0 if m == 0 else 2.0)
        t = tw[(j * m) % L]
        for q in range(2):
            x = (x + (G[q][:, m, :, None] * (cm * t[None, None, :, q])).astype(f32)).astype(f32)
    return x


def _fma(acc, a, b):
    return (acc + (a * b).astype(f32)).astype(f32)


def emulate_synthesis(A, B, rpsi, rchi, kind, nlat, L, T):
    """(u, v) float32 (F, nlat, L) of packed complex64 coefficients A, B (F, rows; either None)"""
    D, Q = (t.astype(f32) for t in dense_tables(kind, nlat, T))
    first = A if A is not None else B
    F = first.shape[0]
    pots = []
    for c, r in ((A, rpsi), (B, rchi)):
        if c is None:
            pots.append(None)
            continue
        a = S.unpack(np.asarray(c, dtype=np.complex64), T)
        r32 = np.ones(T + 1, dtype=f32) if r is None else np.asarray(r, dtype=np.float64).astype(f32)
        re, im = (a.real.astype(f32) * r32).astype(f32), (a.imag.astype(f32) * r32).astype(f32)
        im[:, 0, :] = 0.0
        pots.append((re, im))
    G = np.zeros((2, 2, F, T + 1, nlat), dtype=f32)                  # [u | v][re | im]
    ms = np.arange(T + 1)
    for k0 in range(0, T + 1, 2):
        for which, p in enumerate(pots):
            if p is None:
                continue
            for k in (k0, k0 + 1):
                n = ms + k
                ok = n <= T
                nn = np.where(ok, n, T)
                d = np.where(ok[:, None], D[ms, nn], f32(0))          # [m, i]
                q = np.where(ok[:, None], Q[ms, nn], f32(0))
                re = np.where(ok, p[0][:, ms, nn], f32(0))[:, :, None]        # [F, m, 1]
                im = np.where(ok, p[1][:, ms, nn], f32(0))[:, :, None]
                if which == 0:
                    G[0][0] = _fma(G[0][0], d, -re); G[0][1] = _fma(G[0][1], d, -im)
                    G[1][0] = _fma(G[1][0], q, -im); G[1][1] = _fma(G[1][1], q, re)
                else:
                    G[0][0] = _fma(G[0][0], q, -im); G[0][1] = _fma(G[0][1], q, re)
                    G[1][0] = _fma(G[1][0], d, re); G[1][1] = _fma(G[1][1], d, im)
    return _ifourier(G[0], L), _ifourier(G[1], L)


def emulate_analysis(u, v, response, kind, T, want=('vrt', 'div')):
    """dict of packed complex64 coefficients (F, rows) of float32 fields u, v (F, nlat, L)"""
    u, v = np.asarray(u, dtype=f32), np.asarray(v, dtype=f32)
    F, nlat, L = u.shape
    w = 0.5 * R.weights(kind, nlat)
    D, Q = (np.ascontiguousarray((t * w).astype(f32).transpose(2, 0, 1)) for t in dense_tables(kind, nlat, T))     # [i, m, n]
    U, V = _fourier(u, T), _fourier(v, T)                            # [re | im, F, i, m]
    z = np.zeros((2, F, T + 1, T + 1), dtype=f32)
    d = np.zeros((2, F, T + 1, T + 1), dtype=f32)
    pairs = [[i for i in (32 * s + e, 32 * s + e + 16) if i < nlat] for s in range((nlat + 31) // 32) for e in range(16)]
    for pair in pairs:
        if 'vrt' in want:
            for i in pair:
                z[0] = _fma(z[0], D[i], U[0][:, i, :, None]); z[1] = _fma(z[1], D[i], U[1][:, i, :, None])
            for i in pair:
                z[0] = _fma(z[0], Q[i], -V[1][:, i, :, None]); z[1] = _fma(z[1], Q[i], V[0][:, i, :, None])
        if 'div' in want:
            for i in pair:
                d[0] = _fma(d[0], Q[i], -U[1][:, i, :, None]); d[1] = _fma(d[1], Q[i], U[0][:, i, :, None])
            for i in pair:
                d[0] = _fma(d[0], D[i], -V[0][:, i, :, None]); d[1] = _fma(d[1], D[i], -V[1][:, i, :, None])
    r = np.ones(T + 1, dtype=f32) if response is None else np.asarray(response, dtype=np.float64).astype(f32)
    out = {}
    for name, a in (('vrt', z), ('div', d)):
        if name in want:
            a = ((a.astype(np.float64) / float(L)) * r.astype(np.float64)).astype(f32)
            out[name] = S.pack(a[0] + 1j * a[1]).astype(np.complex64)
    return out


# ---- the barotropic model ------------------------------------------------------------------------------------------------ #

RH = dict(R=4, w=7.848e-6, K=7.848e-6, omega=7.29e-5, radius=6371200.)


def rossby_haurwitz(kind, nlat, L, shift=0.0, K=None, w=None):
    """the vorticity of the Rossby-Haurwitz wave of wavenumber R on the grid (north to south), translated east by `shift` radians"""
    Rw = RH['R']
    K = RH['K'] if K is None else K
    w = RH['w'] if w is None else w
    mu = R.sin_lat(kind, nlat)[:, None]
    c = np.sqrt(1.0 - mu * mu)
    lam = 2 * np.pi * np.arange(L)[None, :] / L
    return 2 * w * mu - K * mu * c ** Rw * (Rw * Rw + 3 * Rw + 2) * np.cos(Rw * (lam - shift))


def rossby_haurwitz_speed():
    Rw, w, Om = RH['R'], RH['w'], RH['omega']
    return (Rw * (3 + Rw) * w - 2 * Om) / ((1 + Rw) * (2 + Rw))


def model_params(T, dt, rc, dc, order, radius, omega, kind, nlat):
    n = np.arange(T + 1, dtype=np.float64)
    damp = dc * (n * (n + 1.0) / max(T * (T + 1.0), 1.0)) ** order
    r_uv = np.zeros(T + 1)
    r_uv[1:] = -radius / (n[1:] * (n[1:] + 1.0))
    return dict(T=T, dt=dt, rc=rc, damp=damp, r_uv=r_uv, r_tend=np.full(T + 1, -1.0 / radius),
                f=2.0 * omega * R.sin_lat(kind, nlat))


def emulate_model(z0, kind, p, snapshots):
    """the device model's step in sequential float32 from the grid vorticity z0 (F, nlat, L): {step: (vrt, u, v) float32 grids}
    for the steps named in `snapshots`"""
    z0 = np.asarray(z0, dtype=f32)
    F, nlat, L = z0.shape
    T = p['T']
    zs = S.emulate_analysis(z0, kind, T)
    zp = zs.copy()
    degree = np.concatenate([np.arange(m, T + 1) for m in range(T + 1)])
    d = p['damp'].astype(f32)[degree]
    dt, rc, fcor = f32(p['dt']), f32(p['rc']), p['f'].astype(f32)[None, :, None]

    def diagnose(c):
        u, v = emulate_synthesis(c, None, p['r_uv'], None, kind, nlat, L, T)
        return S.emulate_synthesis(c, kind, nlat, L), u, v

    def parts(c):
        return np.stack([c.real.astype(f32), c.imag.astype(f32)])

    vg, ug, wg = diagnose(zs)
    out = {}
    if 0 in snapshots:
        out[0] = (vg, ug, wg)
    for step in range(1, max(snapshots) + 1):
        s = (fcor + vg).astype(f32)
        tend = parts(emulate_analysis((s * ug).astype(f32), (s * wg).astype(f32), p['r_tend'], kind, T, want=('div',))['div'])
        z, zq = parts(zs), parts(zp)
        t = (((tend - (d * zq).astype(f32)).astype(f32)) / (f32(1) + (d * dt).astype(f32)).astype(f32)).astype(f32)
        if step == 1:
            new = (z + (dt * t).astype(f32)).astype(f32)
            zf = (z + (rc * (new - z).astype(f32)).astype(f32)).astype(f32)
        else:
            z1 = (z + (rc * (zq - (f32(2) * z).astype(f32)).astype(f32)).astype(f32)).astype(f32)
            new = (zq + ((f32(2) * dt) * t).astype(f32)).astype(f32)
            zf = (z1 + (rc * new).astype(f32)).astype(f32)
        zp = (zf[0] + 1j * zf[1]).astype(np.complex64)
        zs = (new[0] + 1j * new[1]).astype(np.complex64)
        vg, ug, wg = diagnose(zs)
        if step in snapshots:
            out[step] = (vg, ug, wg)
    return out


def relative_errors(got, ref):
    """(max |d vorticity| / max |vorticity|, max |d wind| / max |wind|) of (vrt, u, v) grids against their reference"""
    g = [np.asarray(x, dtype=np.float64) for x in got]
    r = [np.asarray(x, dtype=np.float64) for x in ref]
    wind = max(np.abs(r[1]).max(), np.abs(r[2]).max())
    return (float(np.abs(g[0] - r[0]).max() / np.abs(r[0]).max()),
            float(max(np.abs(g[1] - r[1]).max(), np.abs(g[2] - r[2]).max()) / wind))
