"""
The float64 reference of the spherical-harmonic spectrum (sht_ref.py) and the host tables of DLWP/remap/spharm.py checked against
facts neither produced: the quadratures integrate monomials exactly up to their stated degree and not beyond, the table is
orthonormal, closed-form fields give their closed-form spectra, synthesised band-limited fields are recovered and obey Parseval,
a rotation in longitude leaves S_n alone, and the sequential-fp32 emulation of the kernel's scheme stays within the bound that the
GPU tests impose, on every case of their tables.  No device.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sht_ref as R      # noqa: E402

LAYOUTS = [(k, n) for k in ('clenshaw-curtis', 'gauss') for n in (5, 17, 33, 181)] + [('fejer', n) for n in (8, 16, 180)]


@pytest.mark.parametrize('kind,nlat', LAYOUTS + [('clenshaw-curtis', 2), ('fejer', 2), ('gauss', 2), ('fejer', 5)])
def test_weights(kind, nlat):
    from DLWP.remap import spharm
    w = R.weights(kind, nlat)
    assert abs(w.sum() - 2.0) <= 1e-13 and (w > 0).all()
    if kind == 'gauss':
        assert np.array_equal(np.sort(w), np.sort(np.polynomial.legendre.leggauss(nlat)[1]))
    for south_first in (False, True):
        got_kind, got = spharm.latitude_quadrature(R.latitudes(kind, nlat, south_first))
        assert got_kind == kind
        assert np.abs(got - (w[::-1] if south_first else w)).max() <= 1e-15
    # float32 latitude coordinates are recognised too
    assert spharm.latitude_quadrature(R.latitudes(kind, nlat).astype(np.float32))[0] == kind
    mu = R.sin_lat(kind, nlat)
    top = R.exact_degree(kind, nlat)
    for k in range(0, min(top, 60) + 1):
        exact = 0.0 if k % 2 else 2.0 / (k + 1)
        assert abs((w * mu ** k).sum() - exact) <= 1e-13, (kind, nlat, k)
    # the same in a basis that stays of size one (mu^k near degree 2 nlat is all rounding dust away from the poles): the Chebyshev
    # polynomials T_k(mu) = cos(k arccos mu), int T_k = 2 / (1 - k^2) for even k and 0 for odd k -- and one degree beyond fails
    th = np.arccos(np.clip(mu, -1.0, 1.0))
    for k in range(top + 1):
        assert abs((w * np.cos(k * th)).sum() - (0.0 if k % 2 else 2.0 / (1.0 - k * k))) <= 1e-13, (kind, nlat, k)
    assert (top + 1) % 2 == 0
    assert abs((w * np.cos((top + 1) * th)).sum() - 2.0 / (1.0 - (top + 1.0) ** 2)) > 1e-7, 'exact one degree beyond the stated one'
    assert 2 * R.max_truncation(kind, nlat, 10 ** 6) <= top         # Pbar_n^m Pbar_n'^m has degree <= 2 T


@pytest.mark.parametrize('kind,nlat', LAYOUTS)
def test_table_is_orthonormal(kind, nlat):
    from DLWP.remap import spharm
    T = R.max_truncation(kind, nlat, 10 ** 6)
    t, P = R.table(kind, nlat, T), R.pbar(R.sin_lat(kind, nlat), T)
    assert np.isfinite(t).all()
    worst = max(np.abs(t[m, m:] @ P[m, m:].T - np.eye(T + 1 - m)).max() for m in range(T + 1))
    assert worst <= 1e-12, worst
    # the package's packed tables are these numbers, row by row against a brute-force (m, n) enumeration
    for south_first in (False, True):
        t32, t64 = spharm.legendre_table(R.latitudes(kind, nlat, south_first), T)
        rows = R.packed_rows_brute(T)
        assert t64.shape == (len(rows), nlat) and t32.shape == (len(rows), (nlat + 3) // 4 * 4) and t32.dtype == np.float32
        dense = t[:, :, ::-1] if south_first else t
        for r, (m, n) in enumerate(rows):
            assert spharm.packed_row(m, n, T) == r
            assert np.abs(t64[r] - dense[m, n]).max() <= 1e-15
        assert np.array_equal(t32[:, :nlat], t64.astype(np.float32)) and not t32[:, nlat:].any()
    assert spharm.packed_rows(T) == len(rows)


def _spectrum(x, kind='clenshaw-curtis', T=8):
    return R.power(R.analysis(x, R.table(kind, x.shape[-2], T)))[0]


def test_closed_forms():
    nlat, L, T = 17, 32, 8
    lat = np.radians(R.latitudes('clenshaw-curtis', nlat))[:, None]
    lon = (2 * np.pi * np.arange(L) / L)[None, :]
    one = np.ones((nlat, L))
    for x, want in ((-2.5 * one, {0: 6.25}), (np.sin(lat) * one, {1: 1 / 3}), (np.cos(lat) * np.cos(lon), {1: 1 / 3})):
        S = _spectrum(x)
        ref = np.zeros(T + 1)
        for n, val in want.items():
            ref[n] = val
        assert np.abs(S - ref).max() <= 1e-14
    for n, m in ((0, 0), (3, 0), (5, 2), (8, 8), (8, 1)):
        a = np.zeros((T + 1, T + 1), dtype=complex)
        a[m, n] = 0.7 if m == 0 else 0.3 - 0.4j
        S = _spectrum(R.synthesis(a, 'clenshaw-curtis', nlat, L))
        want = np.zeros(T + 1)
        want[n] = 0.49 if m == 0 else 2 * 0.25
        assert np.abs(S - want).max() <= 1e-13, (n, m)


@pytest.mark.parametrize('kind,nlat,L', [('clenshaw-curtis', 17, 32), ('clenshaw-curtis', 33, 70), ('fejer', 16, 36), ('gauss', 24, 50),
                                         ('gauss', 5, 9)])
def test_recovery_parseval_and_rotation(kind, nlat, L):
    rng = np.random.default_rng(nlat + L)
    T = R.max_truncation(kind, nlat, L)
    t = R.table(kind, nlat, T)
    a = R.random_coefficients(rng, T, slope=1.0)
    x = R.synthesis(a, kind, nlat, L)
    got = R.analysis(x, t)
    scale = np.abs(a).max()
    assert np.abs(got - a).max() <= 1e-11 * scale
    S = R.power(got)[0]
    assert abs(S.sum() - R.mean_square(x, kind)) <= 1e-11 * S.sum()
    assert abs(S[0] - a[0, 0].real ** 2) <= 1e-11 * S.sum()
    for shift in (1, L // 3):
        assert np.abs(R.power(R.analysis(np.roll(x, shift, axis=-1), t))[0] - S).max() <= 1e-12 * S.max()
    # the pair form against itself and against an unrelated field
    y = R.synthesis(R.random_coefficients(rng, T), kind, nlat, L)
    q = R.power(got, R.analysis(y, t))
    assert np.abs(q[0] - S).max() == 0 and (q[2] ** 2 <= q[0] * q[1] * (1 + 1e-12)).all()
    assert np.abs(R.power(got, got)[2] - S).max() <= 1e-15 * S.max()


def test_host_transform_is_the_reference():
    from DLWP.remap import spharm
    rng = np.random.default_rng(3)
    for kind, nlat, L, T in R.EMULATED[:4]:
        f, v = R.make_field(rng, (2, 3, nlat, L)), R.make_field(rng, (2, 3, nlat, L), 'red')
        for south_first in (False, True):
            tr = spharm.SphericalTransform(R.latitudes(kind, nlat, south_first), L, T)
            assert (tr.kind, tr.truncation) == (kind, T)
            ref, _, _ = R.reference(f, v, kind, T, south_first=south_first)
            assert np.abs(tr.power(f, v) - ref).max() <= 1e-13 * np.abs(ref).max()
        assert spharm.SphericalTransform(R.latitudes(kind, nlat), L).truncation == R.max_truncation(kind, nlat, L)


@pytest.mark.parametrize('case', R.EMULATED, ids=lambda c: '%s-%dx%d-T%d' % c)
def test_emulation_within_bound_five_cases(case):
    kind, nlat, L, T = case
    rng = np.random.default_rng(nlat)
    worst = 0.0
    for fk, off in (('white', 0.0), ('white', 300.0), ('red', 0.0)):
        f, v = R.make_field(rng, (2, nlat, L), fk, off), R.make_field(rng, (2, nlat, L), fk, off)
        ref, _, lim = R.reference(f, v, kind, T)
        frac = (np.abs(R.emulate(f, v, kind, T) - ref) / lim).max()
        worst = max(worst, frac)
        assert frac <= 1.0
    print('%s %d x %d T = %d: largest fraction of the bound = %.4f' % (kind, nlat, L, T, worst))


def test_emulation_within_bound_gpu_tables():
    """the reference alone satisfies the condition the GPU tests impose: every case of their grid, and the tile-edge truncations"""
    rng = np.random.default_rng(5)
    cases = R.grid_cases() + [('gauss', 48, 96, T, 3, True) for T in R.GPU_T_EDGE]
    assert len(R.grid_cases()) >= 2 * len(R.GPU_NLAT) * len(R.GPU_L) - 8
    assert set(c[4] for c in cases) == set(R.GPU_FIELDS) and set(c[0] for c in cases) == set(R.KINDS)
    worst = 0.0
    for kind, nlat, L, T, fields, pair in cases:
        fields = min(fields, 3)                                     # the emulation is per field: three of them say as much
        f = R.make_field(rng, (fields, nlat, L), 'white', 280.0 if pair else 0.0)
        v = R.make_field(rng, (fields, nlat, L), 'red') if pair else None
        ref, _, lim = R.reference(f, v, kind, T)
        err = np.abs(R.emulate(f, v, kind, T) - ref)
        assert (err <= lim).all(), (kind, nlat, L, T)
        worst = max(worst, float((err / np.maximum(lim, np.finfo(float).tiny)).max()))
    print('largest fraction of the bound over the GPU tables = %.4f' % worst)


def test_groups_and_dims_against_brute_force():
    from DLWP import ops
    for lead, red in (((3, 4), {1}), ((3, 4), {0}), ((2, 3, 4), {0, 2}), ((2, 3, 4), {1}), ((5,), set()), ((2, 1, 3), {1}),
                      ((2, 3), {0, 1})):
        gs, ri = ops.sht_groups_host(lead, red)
        want = R.groups_reference(lead, red)
        assert gs.tolist() == list(np.cumsum([0] + [len(g) for g in want]))
        assert [ri[gs[k]:gs[k + 1]].tolist() for k in range(len(want))] == want
    # merged leading dims address every field where a row-major walk over the logical shape finds it
    import spectrum_ref as Z
    shape, strides = (3, 5, 2, 7), [(5 * 2 * 7 * 40, 2 * 7 * 40, 7 * 40, 40), (1000, 100, 21, 3)]
    dims = ops.spectrum_dims(shape, strides, ())
    assert len(dims) == 3                               # only the last two axes merge in both operands
    got = Z.dims_offsets(dims, 2)
    want = Z.spectrum_dims_reference(shape, strides, set())
    assert np.array_equal(got.reshape(2, -1), want.reshape(2, -1))
