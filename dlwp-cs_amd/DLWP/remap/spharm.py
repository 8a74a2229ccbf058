"""
Spherical-harmonic analysis on lat-lon grids: the quadratures, the Legendre table and the host transform behind
DLWP.verify.spherical_spectrum (device: ops.spherical_spectrum / dlwpcs_sht_spectrum, include/dlwpcs.h).  numpy only; torch is
touched by SphericalTransform.device_tables alone.

A field x[i, j] lies on nlat latitudes (mu_i = sin(lat_i), weights w_i >= 0 with sum w_i = 2) and L equally spaced longitudes.
Pbar_n^m are the associated Legendre functions with (1/2) int Pbar_n^m Pbar_n'^m dmu = delta_nn' (no Condon-Shortley phase):
    X_m(i) = sum_j x[i,j] exp(-2 pi i j m / L),   a_n^m = sum_i (w_i / 2) Pbar_n^m(mu_i) X_m(i) / L      (0 <= m <= n <= T)
    S_n    = sum_{m=0..n} c_m |a_n^m|^2,   c_0 = 1, c_m = 2 otherwise.
For a field band-limited to T, sum_n S_n is its area-weighted mean square; S_0 is the squared global mean.
Synthesis with a real response r_n (device: ops.spherical_synthesis / dlwpcs_sht_synthesis):
    x[i, j] = sum_{m=0..T} c_m Re( exp(+2 pi i j m / L) sum_{n=m..T} r_n a_n^m Pbar_n^m(mu_i) );   Im a_n^0 is ignored,
and synthesis(analysis(x)) = x for a field band-limited to T.  Coefficients are packed in the order of packed_row(m, n, T).

Vector harmonics (device: ops.spherical_vector_synthesis / spherical_vector_analysis, dlwpcs_sht_vector_*).  With phi the latitude,
D_n^m = dPbar_n^m / dphi and Q_n^m = m Pbar_n^m / cos(phi) (derivative_table, zonal_table; their limits at a pole row), potentials
psi_n^m = rpsi_n A_n^m, chi_n^m = rchi_n B_n^m give the wind u = -dpsi/dphi + (1/cos) dchi/dlambda, v = (1/cos) dpsi/dlambda + dchi/dphi:
    U_m(i) = sum_n [-D psi + i Q chi],   V_m(i) = sum_n [i Q psi + D chi],   then the inverse Fourier stage of the synthesis,
and a wind gives  vrt_n^m = r_n sum_i (w_i / 2) [i Q V_m + D U_m] / L,   div_n^m = r_n sum_i (w_i / 2) [i Q U_m - D V_m] / L.
The factor 1 / radius lives in the responses (uv_from_vrtdiv, vrtdiv_from_uv, gradient put it there).  The largest truncation of
the scalar transform serves the vector forms too.

Three latitude layouts are recognised (either direction):
    'gauss'            the nodes of numpy.polynomial.legendre.leggauss(nlat); exact for T <= nlat - 1
    'clenshaw-curtis'  equally spaced with both poles; exact while 2 T <= nlat - 1
    'fejer'            equally spaced cell centres (LatLonGrid.cells); exact while 2 T <= nlat - 1
and every layout needs L >= 2 T + 1.
"""
import numpy as np

KINDS = ('gauss', 'clenshaw-curtis', 'fejer')
LAT_TOL = 1e-4              # degrees: latitude coordinates are often stored as float32


def _nodes(kind, nlat):
    """(colatitude in radians north to south or None, mu = sin(latitude) north to south) of a layout"""
    if kind == 'gauss':
        mu = -np.polynomial.legendre.leggauss(nlat)[0]
        return None, mu
    i = np.arange(nlat, dtype=np.float64)
    theta = i * np.pi / (nlat - 1) if kind == 'clenshaw-curtis' else (2.0 * i + 1.0) * np.pi / (2.0 * nlat)
    mu = np.cos(theta)
    if kind == 'clenshaw-curtis':
        mu[0], mu[-1] = 1.0, -1.0
    return theta, mu


def _weights(kind, nlat):
    """the quadrature weights north to south, float64, summing to 2"""
    if kind == 'gauss':
        return np.polynomial.legendre.leggauss(nlat)[1][::-1].copy()
    theta, _ = _nodes(kind, nlat)
    if kind == 'clenshaw-curtis':
        N = nlat - 1
        c = np.full(nlat, 2.0)
        c[0] = c[-1] = 1.0
        s = np.zeros(nlat)
        for k in range(1, N // 2 + 1):
            s += (1.0 if 2 * k == N else 2.0) * np.cos(2 * k * theta) / (4.0 * k * k - 1.0)
        return c / N * (1.0 - s)
    s = np.zeros(nlat)
    for k in range(1, nlat // 2 + 1):
        s += np.cos(2 * k * theta) / (4.0 * k * k - 1.0)
    return 2.0 / nlat * (1.0 - 2.0 * s)


def _classify(lat):
    """(kind, flipped): the layout of a latitude vector in degrees; flipped when it runs south to north"""
    lat = np.asarray(getattr(lat, 'values', lat), dtype=np.float64).reshape(-1)
    nlat = lat.size
    if nlat < 2 or not np.all(np.isfinite(lat)):
        raise ValueError('latitude_quadrature: at least 2 finite latitudes are needed')
    flipped = bool(lat[0] < lat[-1])
    d = lat[::-1] if flipped else lat
    for kind in ('clenshaw-curtis', 'fejer', 'gauss'):
        if kind == 'clenshaw-curtis':
            want = 90.0 - 180.0 * np.arange(nlat) / (nlat - 1)
        elif kind == 'fejer':
            want = 90.0 - 180.0 * (2.0 * np.arange(nlat) + 1.0) / (2.0 * nlat)
        else:
            want = np.degrees(np.arcsin(_nodes(kind, nlat)[1]))
        if np.abs(d - want).max() <= LAT_TOL:
            return kind, flipped
    raise ValueError('latitude_quadrature: %d latitudes from %g to %g are neither Gaussian nor equally spaced with both poles '
                     'nor equally spaced cell centres' % (nlat, lat[0], lat[-1]))


def latitude_quadrature(lat):
    """(kind, weights): the layout of the latitude vector `lat` (degrees, either direction) -- 'gauss', 'clenshaw-curtis' or
    'fejer' -- and its float64 quadrature weights in the order of `lat`, w_i >= 0, sum w_i = 2.  Any other vector is refused."""
    kind, flipped = _classify(lat)
    w = _weights(kind, np.asarray(getattr(lat, 'values', lat)).size)
    return kind, (w[::-1].copy() if flipped else w)


def max_truncation(kind, nlat, n_lon):
    """the largest truncation the quadrature and the longitudes allow"""
    t_lat = nlat - 1 if kind == 'gauss' else (nlat - 1) // 2
    return max(min(t_lat, (int(n_lon) - 1) // 2), 0)


def packed_rows(T):
    return (T + 1) * (T + 2) // 2


def packed_row(m, n, T):
    """row of (m, n) in the packed table: orders outermost, within an order the degrees n = m .. T"""
    return m * (T + 1) - m * (m - 1) // 2 + (n - m)


def legendre_functions(mu, T):
    """Pbar_n^m(mu_i) for 0 <= m <= n <= T, packed rows x len(mu), float64, by the three-term recurrence in n"""
    mu = np.asarray(mu, dtype=np.float64)
    cos_lat = np.sqrt(np.maximum(1.0 - mu * mu, 0.0))
    P = np.zeros((packed_rows(T), mu.size))
    pmm = np.ones(mu.size)
    for m in range(T + 1):
        if m > 0:
            pmm = np.sqrt((2.0 * m + 1.0) / (2.0 * m)) * cos_lat * pmm
        r = packed_row(m, m, T)
        P[r] = pmm
        if m < T:
            P[r + 1] = np.sqrt(2.0 * m + 3.0) * mu * pmm
        for n in range(m + 2, T + 1):
            A = np.sqrt((4.0 * n * n - 1.0) / (n * n - m * m))
            B = np.sqrt(((n - 1.0) ** 2 - m * m) / (4.0 * (n - 1.0) ** 2 - 1.0))
            P[r + n - m] = A * (mu * P[r + n - m - 1] - B * P[r + n - m - 2])
    return P


def legendre_table(lat, truncation):
    """(float32 packed table (rows, nlat padded with zeros to a multiple of 4), its float64 parent (rows, nlat)):
    (w_i / 2) Pbar_n^m(mu_i) in the order of `lat`, row packed_row(m, n, T); every entry evaluated in float64 and rounded once"""
    kind, flipped = _classify(lat)
    nlat = np.asarray(getattr(lat, 'values', lat)).size
    T = int(truncation)
    if T < 0 or T > (nlat - 1 if kind == 'gauss' else (nlat - 1) // 2):
        raise ValueError("legendre_table: truncation %d is outside what %d '%s' latitudes integrate exactly (0 .. %d)"
                         % (T, nlat, kind, nlat - 1 if kind == 'gauss' else (nlat - 1) // 2))
    mu, w = _nodes(kind, nlat)[1], _weights(kind, nlat)
    t64 = legendre_functions(mu, T) * (0.5 * w)[None, :]
    if flipped:
        t64 = np.ascontiguousarray(t64[:, ::-1])
    t32 = np.zeros((t64.shape[0], (nlat + 3) // 4 * 4), dtype=np.float32)
    t32[:, :nlat] = t64
    return t32, t64


def unweighted_table(lat, truncation):
    """(float32 packed table (rows, nlat padded with zeros to a multiple of 4), its float64 parent (rows, nlat)): Pbar_n^m(mu_i)
    in the order of `lat`, the packing of legendre_table; every entry evaluated in float64 and rounded once (it is not the
    weighted table divided by the weights: that would round twice)"""
    kind, flipped = _classify(lat)
    nlat = np.asarray(getattr(lat, 'values', lat)).size
    p64 = legendre_functions(_nodes(kind, nlat)[1], int(truncation))
    if flipped:
        p64 = np.ascontiguousarray(p64[:, ::-1])
    p32 = np.zeros((p64.shape[0], (nlat + 3) // 4 * 4), dtype=np.float32)
    p32[:, :nlat] = p64
    return p32, p64


def _vector_functions(kind, nlat, T):
    """(D, Q) north to south, float64 (packed rows of T, nlat): D_n^m = dPbar_n^m / dphi and Q_n^m = m Pbar_n^m / cos(phi), with their
    limits at a pole row (zero but for m = 1, where p_n = Pbar_n^1 / cos(phi) gives Q = p_n and D = -mu p_n)"""
    mu = _nodes(kind, nlat)[1]
    cos_lat = np.sqrt(np.maximum(1.0 - mu * mu, 0.0))
    pole = cos_lat == 0.0
    inv_cos = 1.0 / np.where(pole, 1.0, cos_lat)
    P = legendre_functions(mu, T + 1)
    D, Q = np.zeros((packed_rows(T), nlat)), np.zeros((packed_rows(T), nlat))
    for m in range(T + 1):
        r, r1 = packed_row(m, m, T), packed_row(m, m, T + 1)
        for n in range(m, T + 1):
            e1 = np.sqrt(((n + 1.0) ** 2 - m * m) / (4.0 * (n + 1.0) ** 2 - 1.0))
            d = -n * e1 * P[r1 + n + 1 - m]
            if n > m:
                d = d + (n + 1.0) * np.sqrt((n * n - m * m) / (4.0 * n * n - 1.0)) * P[r1 + n - 1 - m]
            D[r + n - m] = d * inv_cos
            Q[r + n - m] = m * P[r1 + n - m] * inv_cos
    if pole.any():
        D[:, pole], Q[:, pole] = 0.0, 0.0
        if T >= 1:
            x = mu[pole]
            p = np.zeros((T + 1, x.size))               # p_n = Pbar_n^1 / cos(phi): the recurrence of legendre_functions, m = 1
            p[1] = np.sqrt(1.5)
            if T >= 2:
                p[2] = np.sqrt(5.0) * x * p[1]
            for n in range(3, T + 1):
                A = np.sqrt((4.0 * n * n - 1.0) / (n * n - 1.0))
                B = np.sqrt(((n - 1.0) ** 2 - 1.0) / (4.0 * (n - 1.0) ** 2 - 1.0))
                p[n] = A * (x * p[n - 1] - B * p[n - 2])
            r = packed_row(1, 1, T)
            Q[r:r + T, pole] = p[1:]
            D[r:r + T, pole] = -x * p[1:]
    return D, Q


def _vector_table(lat, truncation, which, weighted):
    kind, flipped = _classify(lat)
    nlat = np.asarray(getattr(lat, 'values', lat)).size
    T = int(truncation)
    if T < 0 or T > (nlat - 1 if kind == 'gauss' else (nlat - 1) // 2):
        raise ValueError("%s_table: truncation %d is outside what %d '%s' latitudes integrate exactly (0 .. %d)"
                         % (('derivative', 'zonal')[which], T, nlat, kind, nlat - 1 if kind == 'gauss' else (nlat - 1) // 2))
    t64 = _vector_functions(kind, nlat, T)[which]
    if weighted:
        t64 = t64 * (0.5 * _weights(kind, nlat))[None, :]
    if flipped:
        t64 = np.ascontiguousarray(t64[:, ::-1])
    t32 = np.zeros((t64.shape[0], (nlat + 3) // 4 * 4), dtype=np.float32)
    t32[:, :nlat] = t64
    return t32, t64


def derivative_table(lat, truncation, weighted=False):
    """(float32 packed table (rows, nlat padded with zeros to a multiple of 4), its float64 parent (rows, nlat)):
    D_n^m(mu_i) = dPbar_n^m / dphi = [-n eps_{n+1}^m Pbar_{n+1}^m + (n + 1) eps_n^m Pbar_{n-1}^m] / cos(phi_i),
    eps_n^m = sqrt((n^2 - m^2) / (4 n^2 - 1)), in the order of `lat` and the packing of legendre_table; weighted: times w_i / 2.
    Every entry is evaluated in float64 and rounded once.  At a pole row the entry is the limit: -mu p_n for m = 1 with
    p_n = Pbar_n^1 / cos(phi), zero otherwise."""
    return _vector_table(lat, truncation, 0, weighted)


def zonal_table(lat, truncation, weighted=False):
    """as derivative_table, for Q_n^m(mu_i) = m Pbar_n^m(mu_i) / cos(phi_i); at a pole row p_n for m = 1, zero otherwise"""
    return _vector_table(lat, truncation, 1, weighted)


VECTOR_TABLES = ('D', 'Q', 'wD', 'wQ')


def truncation_response(T, cutoff):
    """(T + 1,) float64: 1 for the degrees n <= cutoff, 0 above"""
    T, cutoff = int(T), int(cutoff)
    if T < 0 or cutoff < 0:
        raise ValueError('truncation_response: T = %d, cutoff = %d (both at least 0)' % (T, cutoff))
    return (np.arange(T + 1) <= cutoff).astype(np.float64)


def laplacian_response(T, radius=6371200., inverse=False):
    """(T + 1,) float64: -n (n + 1) / radius^2, the Laplacian on a sphere of `radius` metres in spectral space; inverse: its
    reciprocal, with 0 at n = 0 (the mean is lost)"""
    n = np.arange(int(T) + 1, dtype=np.float64)
    r = -n * (n + 1.0) / float(radius) ** 2
    if inverse:
        r[1:] = 1.0 / r[1:]
    return r


def uv_response(T, radius=6371200.):
    """(T + 1,) float64: -radius / (n (n + 1)), 0 at n = 0: vorticity (divergence) to the streamfunction (velocity potential)
    times 1 / radius, the response of uv_from_vrtdiv"""
    n = np.arange(int(T) + 1, dtype=np.float64)
    r = np.zeros(int(T) + 1)
    r[1:] = -float(radius) / (n[1:] * (n[1:] + 1.0))
    return r


class SphericalTransform(object):
    """The analysis of fields on `lat` (degrees) x n_lon longitudes up to `truncation` (None: the largest the grid allows):
    kind, weights, truncation, the packed tables, and one device copy of the float32 table and the twiddles per device."""

    def __init__(self, lat, n_lon, truncation=None):
        self.lat = np.asarray(getattr(lat, 'values', lat), dtype=np.float64).reshape(-1).copy()
        self.kind, self.weights = latitude_quadrature(self.lat)
        self.nlat, self.n_lon = self.lat.size, int(n_lon)
        if self.n_lon < 2:
            raise ValueError('SphericalTransform: %d longitudes (at least 2)' % self.n_lon)
        most = max_truncation(self.kind, self.nlat, self.n_lon)
        if truncation is None:
            truncation = most
        T = int(truncation)
        if T < 0:
            raise ValueError('SphericalTransform: truncation %d is negative' % T)
        if 2 * T + 1 > self.n_lon:
            raise ValueError('SphericalTransform: truncation %d needs at least %d longitudes, the grid has %d'
                             % (T, 2 * T + 1, self.n_lon))
        if T > most:
            raise ValueError("SphericalTransform: truncation %d is above %d, the largest that %d '%s' latitudes integrate exactly"
                             % (T, most, self.nlat, self.kind))
        self.truncation = T
        self.table32, self.table64 = legendre_table(self.lat, T)
        self._device = {}
        self._unweighted, self._device_unweighted = None, {}
        self._vector, self._device_vector = None, {}

    def device_tables(self, device):
        """(twiddle table, Legendre table) on `device`, uploaded at the first use there (not inside a graph capture)"""
        import torch
        from .. import ops
        key = str(torch.device(device))
        hit = self._device.get(key)
        if hit is None:
            if torch.cuda.is_current_stream_capturing():
                raise ops.nat.NativeError('spherical_spectrum: first use of this transform inside a graph capture (run it once '
                                          'eagerly first)')
            hit = (ops.spectrum_twiddle(self.n_lon, device), torch.from_numpy(self.table32).to(device))
            self._device[key] = hit
        return hit

    def synthesis_tables(self):
        """(float32, float64) unweighted tables Pbar_n^m(mu_i) of the synthesis, made at the first use"""
        if self._unweighted is None:
            self._unweighted = unweighted_table(self.lat, self.truncation)
        return self._unweighted

    def device_synthesis_tables(self, device):
        """(twiddle table, unweighted Legendre table) on `device`, uploaded at the first use there (not inside a graph capture)"""
        import torch
        from .. import ops
        key = str(torch.device(device))
        hit = self._device_unweighted.get(key)
        if hit is None:
            if torch.cuda.is_current_stream_capturing():
                raise ops.nat.NativeError('spherical_synthesis: first use of this transform inside a graph capture (run it once '
                                          'eagerly first)')
            hit = (ops.spectrum_twiddle(self.n_lon, device), torch.from_numpy(self.synthesis_tables()[0]).to(device))
            self._device_unweighted[key] = hit
        return hit

    def vector_tables(self):
        """dict of the (float32, float64) tables 'D', 'Q' (derivative_table, zonal_table) and 'wD', 'wQ' (their weighted forms), made
        at the first use"""
        if self._vector is None:
            self._vector = {'D': derivative_table(self.lat, self.truncation), 'Q': zonal_table(self.lat, self.truncation),
                            'wD': derivative_table(self.lat, self.truncation, weighted=True),
                            'wQ': zonal_table(self.lat, self.truncation, weighted=True)}
        return self._vector

    def device_vector_tables(self, device):
        """(twiddle table, D, Q, wD, wQ) on `device`, uploaded at the first use there (not inside a graph capture)"""
        import torch
        from .. import ops
        key = str(torch.device(device))
        hit = self._device_vector.get(key)
        if hit is None:
            if torch.cuda.is_current_stream_capturing():
                raise ops.nat.NativeError('spherical_vector: first use of this transform inside a graph capture (run it once '
                                          'eagerly first)')
            t = self.vector_tables()
            hit = (ops.spectrum_twiddle(self.n_lon, device),) + tuple(torch.from_numpy(t[k][0]).to(device) for k in VECTOR_TABLES)
            self._device_vector[key] = hit
        return hit

    def _response(self, r):
        T = self.truncation
        r = np.ones(T + 1) if r is None else np.asarray(r, dtype=np.float64).reshape(-1)
        if r.shape != (T + 1,):
            raise ValueError('SphericalTransform: a response of %d factors, truncation %d needs %d' % (r.size, T, T + 1))
        return r

    def vector_synthesis(self, A=None, B=None, rpsi=None, rchi=None):
        """(u, v) float64 (..., nlat, n_lon) of the potentials psi_n^m = rpsi_n A_n^m and chi_n^m = rchi_n B_n^m (complex, packed;
        either may be None, not both):  u = -dpsi/dphi + (1/cos) dchi/dlambda,  v = (1/cos) dpsi/dlambda + dchi/dphi,  per order
        U_m = sum_n [-D psi + i Q chi],  V_m = sum_n [i Q psi + D chi].  The factor 1 / radius belongs in the responses.
        Im of order 0 is ignored."""
        if A is None and B is None:
            raise ValueError('SphericalTransform: vector_synthesis needs a potential')
        T, L = self.truncation, self.n_lon
        pots = []
        for c, r in ((A, rpsi), (B, rchi)):
            if c is None:
                pots.append(None)
                continue
            c = np.asarray(c, dtype=np.complex128)
            if c.shape[-1:] != (packed_rows(T),):
                raise ValueError('SphericalTransform: %s coefficients per field, truncation %d has %d'
                                 % (c.shape[-1:], T, packed_rows(T)))
            pots.append((c, self._response(r)))
        if pots[0] is not None and pots[1] is not None and pots[0][0].shape != pots[1][0].shape:
            raise ValueError('SphericalTransform: the two potentials must have one shape')
        t = self.vector_tables()
        D, Q = t['D'][1], t['Q'][1]
        lead = (pots[0] or pots[1])[0].shape[:-1]
        U = np.zeros(lead + (self.nlat, L // 2 + 1), dtype=np.complex128)
        V = np.zeros_like(U)
        for m in range(T + 1):
            s = packed_row(m, m, T)
            sl = slice(s, s + T + 1 - m)
            if pots[0] is not None:
                a = pots[0][0][..., sl] * pots[0][1][m:]
                if m == 0:
                    a = a.real.astype(np.complex128)
                U[..., m] -= np.einsum('ni,...n->...i', D[sl], a)
                V[..., m] += 1j * np.einsum('ni,...n->...i', Q[sl], a)
            if pots[1] is not None:
                b = pots[1][0][..., sl] * pots[1][1][m:]
                if m == 0:
                    b = b.real.astype(np.complex128)
                U[..., m] += 1j * np.einsum('ni,...n->...i', Q[sl], b)
                V[..., m] += np.einsum('ni,...n->...i', D[sl], b)
        return np.fft.irfft(U * L, n=L, axis=-1), np.fft.irfft(V * L, n=L, axis=-1)

    def vector_analysis(self, u, v, response=None, want=('vrt', 'div')):
        """the coefficients named in `want` ('vrt', 'div'; a tuple in that order) of the float64 fields u, v (..., nlat, n_lon):
        zeta_n^m = r_n sum_i (w_i / 2) [i Q V_m + D U_m] / L,  delta_n^m = r_n sum_i (w_i / 2) [i Q U_m - D V_m] / L, complex
        (..., packed rows).  response: T + 1 real factors (None: ones; 1 / radius for vorticity and divergence)."""
        want = (want,) if isinstance(want, str) else tuple(want)
        if not want or any(w not in ('vrt', 'div') for w in want) or len(set(want)) != len(want):
            raise ValueError("SphericalTransform: want %s, a non-empty choice of ('vrt', 'div')" % (want,))
        u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
        if u.shape != v.shape or u.shape[-2:] != (self.nlat, self.n_lon):
            raise ValueError('SphericalTransform: fields of %s and %s, the transform is for %s'
                             % (u.shape, v.shape, (self.nlat, self.n_lon)))
        T = self.truncation
        r = self._response(response)
        t = self.vector_tables()
        wD, wQ = t['wD'][1], t['wQ'][1]
        U = np.fft.rfft(u, axis=-1)[..., :T + 1] / self.n_lon
        V = np.fft.rfft(v, axis=-1)[..., :T + 1] / self.n_lon
        out = {w: np.empty(u.shape[:-2] + (packed_rows(T),), dtype=np.complex128) for w in want}
        for m in range(T + 1):
            s = packed_row(m, m, T)
            sl = slice(s, s + T + 1 - m)
            if 'vrt' in out:
                out['vrt'][..., sl] = r[m:] * (1j * np.einsum('ni,...i->...n', wQ[sl], V[..., m])
                                               + np.einsum('ni,...i->...n', wD[sl], U[..., m]))
            if 'div' in out:
                out['div'][..., sl] = r[m:] * (1j * np.einsum('ni,...i->...n', wQ[sl], U[..., m])
                                               - np.einsum('ni,...i->...n', wD[sl], V[..., m]))
        return tuple(out[w] for w in want)

    def uv_from_vrtdiv(self, vrt=None, div=None, radius=6371200.):
        """(u, v) of the vorticity and divergence coefficients (either may be None): psi = lap^-1 zeta, chi = lap^-1 delta"""
        return self.vector_synthesis(vrt, div, uv_response(self.truncation, radius), uv_response(self.truncation, radius))

    def vrtdiv_from_uv(self, u, v, radius=6371200., want=('vrt', 'div')):
        """the vorticity and divergence coefficients of the wind (u, v) on a sphere of `radius` metres"""
        return self.vector_analysis(u, v, np.full(self.truncation + 1, 1.0 / float(radius)), want)

    def gradient(self, coef, radius=6371200.):
        """(ds/dlambda / (radius cos), ds/dphi / radius) of the scalar with the coefficients `coef`"""
        return self.vector_synthesis(None, coef, None, np.full(self.truncation + 1, 1.0 / float(radius)))

    def synthesis(self, coef, response=None):
        """x[i, j] = sum_m c_m Re(e^{2 pi i j m / L} sum_n r_n a_n^m Pbar_n^m(mu_i)) of complex coefficients (..., packed rows):
        float64 (..., nlat, n_lon).  response: T + 1 real factors per degree (None: ones).  Im a_n^0 is ignored."""
        coef = np.asarray(coef, dtype=np.complex128)
        T, L = self.truncation, self.n_lon
        if coef.shape[-1:] != (packed_rows(T),):
            raise ValueError('SphericalTransform: %s coefficients per field, truncation %d has %d'
                             % (coef.shape[-1:], T, packed_rows(T)))
        r = np.ones(T + 1) if response is None else np.asarray(response, dtype=np.float64).reshape(-1)
        if r.shape != (T + 1,):
            raise ValueError('SphericalTransform: a response of %d factors, truncation %d needs %d' % (r.size, T, T + 1))
        p64 = self.synthesis_tables()[1]
        G = np.zeros(coef.shape[:-1] + (self.nlat, L // 2 + 1), dtype=np.complex128)
        for m in range(T + 1):
            s = packed_row(m, m, T)
            a = coef[..., s:s + T + 1 - m] * r[m:]
            if m == 0:
                a = a.real
            G[..., m] = np.einsum('ni,...n->...i', p64[s:s + T + 1 - m], a)
        # irfft sums c_m Re(G_m e^{i m lon}) / L for 0 < m < L / 2 (T < L / 2 always: L >= 2 T + 1)
        return np.fft.irfft(G * L, n=L, axis=-1)

    def coefficients(self, x):
        """a_n^m of float64 fields x (..., nlat, n_lon): complex (..., packed rows)"""
        x = np.asarray(x, dtype=np.float64)
        if x.shape[-2:] != (self.nlat, self.n_lon):
            raise ValueError('SphericalTransform: fields of %s, the transform is for %s' % (x.shape[-2:], (self.nlat, self.n_lon)))
        T = self.truncation
        X = np.fft.rfft(x, axis=-1)[..., :T + 1] / self.n_lon
        a = np.empty(x.shape[:-2] + (packed_rows(T),), dtype=np.complex128)
        for m in range(T + 1):
            r = packed_row(m, m, T)
            a[..., r:r + T + 1 - m] = np.einsum('ni,...i->...n', self.table64[r:r + T + 1 - m], X[..., m])
        return a

    def power(self, f, v=None):
        """(nq, ..., T + 1) float64: S_n of f; with v also S_n of v and the co-spectrum sum_m c_m Re(a_f conj a_v)"""
        T = self.truncation
        af = self.coefficients(f)
        av = af if v is None else self.coefficients(v)
        prods = [af.real ** 2 + af.imag ** 2]
        if v is not None:
            prods += [av.real ** 2 + av.imag ** 2, (af * np.conj(av)).real]
        out = np.zeros((len(prods),) + af.shape[:-1] + (T + 1,))
        for m in range(T + 1):
            r = packed_row(m, m, T)
            for q, p in enumerate(prods):
                out[q][..., m:] += (1.0 if m == 0 else 2.0) * p[..., r:r + T + 1 - m]
        return out
