"""
The references, bounds and emulations of sht_vector_ref.py checked against facts they did not produce, on the host: the tables
against finite differences and against values just inside the pole, the host twin (DLWP.remap.spharm.SphericalTransform) against
the independent dense reference, and the derived bounds of both device schemes against a sequential-fp32 emulation over the GPU
case table.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sht_ref as R             # noqa: E402
import sht_synth_ref as S       # noqa: E402
import sht_vector_ref as V      # noqa: E402

from DLWP.remap import spharm   # noqa: E402

TINY = np.finfo(np.float64).tiny


@pytest.mark.parametrize('kind,nlat,T', [('gauss', 12, 11), ('fejer', 21, 10), ('clenshaw-curtis', 21, 10)])
def test_derivative_table_is_the_central_difference(kind, nlat, T):
    lat = R.latitudes(kind, nlat)
    _, d64 = spharm.derivative_table(lat, T)
    _, q64 = spharm.zonal_table(lat, T)
    phi = np.radians(lat)
    inner = np.abs(np.cos(phi)) > 1e-3
    h = 1e-5
    P = lambda p: spharm.legendre_functions(np.sin(p), T)       # noqa: E731
    fd = (P(phi[inner] + h) - P(phi[inner] - h)) / (2 * h)
    scale = np.abs(d64).max()
    assert np.abs(d64[:, inner] - fd).max() <= 1e-8 * scale     # h^2 / 6 |P'''| ~ 1e-10 T^3, plus 1e-16 / h of cancellation
    m = np.concatenate([np.full(T + 1 - mm, mm) for mm in range(T + 1)])
    assert np.abs(q64[:, inner] - m[:, None] * P(phi[inner]) / np.cos(phi[inner])).max() <= 1e-12 * scale
    # the dense tables of the reference module are the same functions
    D, Q = V.dense_tables(kind, nlat, T)
    assert np.abs(S.pack(np.moveaxis(D, -1, 0)) - d64.T).max() <= 1e-12 * scale
    assert np.abs(S.pack(np.moveaxis(Q, -1, 0)) - q64.T).max() <= 1e-12 * scale


def test_pole_limits_are_the_values_just_inside():
    nlat, T = 17, 8
    lat = R.latitudes('clenshaw-curtis', nlat)
    _, d64 = spharm.derivative_table(lat, T)
    _, q64 = spharm.zonal_table(lat, T)
    # D and Q are trigonometric polynomials of degree <= T + 1 in the colatitude, so e radians inside the pole they differ from
    # their limits by at most e (T + 1) max |.| (Bernstein); there the general formula holds (its numerator loses log10(1 / e)
    # digits to cancellation: 1e-11 left)
    e = 1e-5
    scale = max(np.abs(d64).max(), np.abs(q64).max())
    tol = e * (T + 1) * scale
    for i, phi in ((0, np.pi / 2 - e), (nlat - 1, -np.pi / 2 + e)):
        P = R.pbar(np.array([np.sin(phi)]), T + 1)[:, :, 0]                    # [m, n]
        eps = lambda n, m: np.sqrt((n * n - m * m) / (4.0 * n * n - 1.0))      # noqa: E731
        for m in range(T + 1):
            for n in range(m, T + 1):
                d = (-n * eps(n + 1, m) * P[m, n + 1] + ((n + 1) * eps(n, m) * P[m, n - 1] if n > m else 0.0)) / np.cos(phi)
                q = m * P[m, n] / np.cos(phi)
                r = spharm.packed_row(m, n, T)
                assert abs(d64[r, i] - d) <= tol and abs(q64[r, i] - q) <= tol, (m, n)
        assert np.abs(q64[:, i]).max() > 0.1 and np.abs(d64[:, i]).max() > 0.1          # (the limits are not zero for m = 1)
    # the float32 tables are the float64 ones rounded once, padded with zeros; the weighted forms carry w_i / 2
    t32, t64 = spharm.derivative_table(lat, T, weighted=True)
    assert t32.shape == (S.packed_rows(T), 20) and t32.dtype == np.float32
    assert np.array_equal(t32[:, :nlat], t64.astype(np.float32)) and not t32[:, nlat:].any()
    assert np.array_equal(t64, d64 * (0.5 * R.weights('clenshaw-curtis', nlat)))
    assert np.array_equal(spharm.zonal_table(lat[::-1], T)[1], q64[:, ::-1])


@pytest.mark.parametrize('kind,nlat,L', V.ROUND_TRIP)
def test_round_trip_at_the_largest_truncation(kind, nlat, L):
    rng = np.random.default_rng(nlat + L)
    tr = spharm.SphericalTransform(R.latitudes(kind, nlat), L)
    T = tr.truncation
    assert T == R.max_truncation(kind, nlat, L)
    z, d = S.random_packed(rng, T, (2,)), S.random_packed(rng, T, (2,))
    z[:, 0], d[:, 0] = 0.0, 0.0                                  # a wind has no mean vorticity or divergence
    u, v = tr.uv_from_vrtdiv(z, d, radius=1.0)
    z2, d2 = tr.vrtdiv_from_uv(u, v, radius=1.0)
    err = max(np.abs(z2 - z).max(), np.abs(d2 - d).max())
    print('%s %d x %d T=%d: round trip error %.2g' % (kind, nlat, L, T, err))
    assert err <= 1e-11


@pytest.mark.parametrize('kind,nlat,L,T,south', [('gauss', 12, 30, 11, False), ('clenshaw-curtis', 17, 36, 8, True), ('fejer', 14, 20, 6, False)])
def test_host_twin_is_the_dense_reference(kind, nlat, L, T, south):
    rng = np.random.default_rng(7)
    tr = spharm.SphericalTransform(R.latitudes(kind, nlat, south), L, T)
    A, B = S.random_packed(rng, T, (3,)), S.random_packed(rng, T, (3,))
    rp, rc = rng.standard_normal(T + 1), rng.standard_normal(T + 1)
    flip = (lambda x: x[..., ::-1, :]) if south else (lambda x: x)
    for a, b in ((A, B), (A, None), (None, B)):
        u, v = tr.vector_synthesis(a, b, rp, rc)
        ru, rv = V.synthesis(a, b, rp, rc, kind, nlat, L, T)
        scale = max(np.abs(ru).max(), np.abs(rv).max())
        assert np.abs(flip(u) - ru).max() <= 1e-12 * scale and np.abs(flip(v) - rv).max() <= 1e-12 * scale
    u, v = rng.standard_normal((3, nlat, L)), rng.standard_normal((3, nlat, L))
    z, d = tr.vector_analysis(u, v, rp)
    rz, rd = V.analysis(flip(u), flip(v), rp, kind, T)
    assert np.abs(z - rz).max() <= 1e-13 and np.abs(d - rd).max() <= 1e-13
    assert np.array_equal(tr.vector_analysis(u, v, rp, want=('div',))[0], d)
    assert np.array_equal(tr.vector_analysis(u, v, rp, want=('div', 'vrt'))[1], z)


def test_the_bounds_hold_for_a_sequential_fp32_evaluation():
    """Over the GPU case table the sequential-fp32 emulation of both schemes stays below the derived bounds.  Measured: the
    synthesis at most 0.20 of its bound, the analysis at most 0.05."""
    worst = [0.0, 0.0]
    for n, (kind, nlat, L, T, fields, _) in enumerate(V.GPU_CASES):
        rng = np.random.default_rng(100 + n)
        F = min(fields, 3)
        A = S.random_packed(rng, T, (F,), slope=(n % 3) * 0.5).astype(np.complex64)
        B = S.random_packed(rng, T, (F,), slope=(n % 2) * 0.5).astype(np.complex64)
        rp = (rng.standard_normal(T + 1)).astype(np.float32) if n % 2 else None
        rc = (rng.standard_normal(T + 1)).astype(np.float32) if n % 3 else None
        a, b = [(A, B), (A, None), (None, B)][n % 3]
        got = V.emulate_synthesis(a, b, rp, rc, kind, nlat, L, T)
        ref = V.synthesis(a, b, rp, rc, kind, nlat, L, T)
        lim = V.synthesis_bound(a, b, rp, rc, kind, nlat, T)
        for g, r, l in zip(got, ref, lim):
            err = np.abs(g.astype(np.float64) - r)
            assert (err <= l[..., None]).all()
            worst[0] = max(worst[0], float((err / np.maximum(l[..., None], TINY)).max()))
        u = R.make_field(rng, (F, nlat, L), 'red' if n % 2 else 'white', 20.0 if n % 3 == 0 else 0.0)
        v = R.make_field(rng, (F, nlat, L), 'white', 0.0)
        got = V.emulate_analysis(u, v, rp, kind, T)
        ref = V.analysis(u.astype(np.float64), v.astype(np.float64), rp, kind, T)
        lim = V.analysis_bound(u.astype(np.float64), v.astype(np.float64), rp, kind, T)
        for g, r, l in zip((got['vrt'], got['div']), ref, lim):
            err = np.maximum(np.abs(g.real.astype(np.float64) - r.real), np.abs(g.imag.astype(np.float64) - r.imag))
            assert (err <= l).all()
            worst[1] = max(worst[1], float((err / np.maximum(l, TINY)).max()))
    print('sequential fp32 / bound: synthesis %.4f, analysis %.4f' % tuple(worst))
    assert worst[0] <= 0.25 and worst[1] <= 0.1              # each scheme its own cap: about twice what it measures
