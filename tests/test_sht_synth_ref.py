"""
The host transform pair of DLWP.remap.spharm (SphericalTransform.coefficients / synthesis, the responses) against facts it did not
produce itself -- scipy's spherical harmonics, the inverse relations, Parseval, the Laplacian's eigenvalues -- and the error bounds
of sht_synth_ref.py against a sequential-fp32 emulation of the device's scheme over the GPU case table.  No device.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sht_ref as R             # noqa: E402
import sht_synth_ref as S       # noqa: E402

from DLWP.remap import spharm   # noqa: E402

GRIDS = [('gauss', 12, 25, 11), ('clenshaw-curtis', 17, 36, 8), ('fejer', 16, 36, 7)]


def _transform(kind, nlat, L, T=None, south_first=False):
    return spharm.SphericalTransform(R.latitudes(kind, nlat, south_first), L, T)


@pytest.mark.parametrize('kind,nlat,L,T', GRIDS)
def test_unit_coefficient_is_scipys_harmonic(kind, nlat, L, T):
    special = pytest.importorskip('scipy.special')
    if not hasattr(special, 'sph_harm_y'):
        pytest.skip('scipy.special.sph_harm_y is not there')
    tr = _transform(kind, nlat, L, T)
    theta, lon = R.colatitudes(kind, nlat), 2 * np.pi * np.arange(L) / L
    worst = 0.0
    for m in range(T + 1):
        for n in range(m, T + 1):
            c = np.zeros(S.packed_rows(T), dtype=np.complex128)
            c[spharm.packed_row(m, n, T)] = 1.0
            Y = special.sph_harm_y(n, m, theta[:, None], lon[None, :])
            want = (1.0 if m == 0 else 2.0) * np.sqrt(4 * np.pi) * (-1.0) ** m * Y.real
            worst = max(worst, np.abs(tr.synthesis(c) - want).max())
    print('%s: largest difference from scipy = %.3g' % (kind, worst))
    assert worst <= 1e-12


@pytest.mark.parametrize('kind,nlat,L,T', GRIDS)
@pytest.mark.parametrize('south_first', [False, True])
def test_the_pair_inverts_itself(kind, nlat, L, T, south_first):
    rng = np.random.default_rng(nlat)
    tr = _transform(kind, nlat, L, T, south_first)
    c = S.random_packed(rng, T, (2, 3))
    x = tr.synthesis(c)
    assert x.shape == (2, 3, nlat, L) and x.dtype == np.float64
    assert np.abs(tr.coefficients(x) - c).max() <= 1e-11                   # analysis o synthesis = identity
    assert np.abs(tr.synthesis(tr.coefficients(x)) - x).max() <= 1e-11     # synthesis o analysis = identity on band-limited fields
    # the independent reference (north to south) agrees with both directions
    ref = S.synthesis(c, kind, nlat, L)
    assert np.abs((x[..., ::-1, :] if south_first else x) - ref).max() <= 1e-11
    assert np.abs(S.analysis(ref, kind, T) - c).max() <= 1e-11
    # Im a_n^0 is ignored
    c2 = c.copy()
    c2[..., :T + 1] += 1j * rng.standard_normal((2, 3, T + 1))
    assert np.array_equal(tr.synthesis(c2), x)
    # sum c_m |a|^2 is the power
    a = S.unpack(c, T)
    want = (R.c_m(T)[:, None] * np.abs(a) ** 2).sum(axis=-2)
    assert np.abs(tr.power(x)[0] - want).max() <= 1e-11 * want.max()


def test_responses():
    T, a = 8, 6371200.
    kind, nlat, L = 'clenshaw-curtis', 17, 36
    tr = _transform(kind, nlat, L, T)
    assert spharm.truncation_response(5, 2).tolist() == [1, 1, 1, 0, 0, 0] and spharm.truncation_response(2, 7).tolist() == [1, 1, 1]
    lap, inv = spharm.laplacian_response(T), spharm.laplacian_response(T, inverse=True)
    n = np.arange(T + 1)
    assert np.allclose(lap, -n * (n + 1) / a ** 2, rtol=1e-15) and inv[0] == 0 and np.allclose(inv[1:] * lap[1:], 1.0, rtol=1e-15)
    assert np.allclose(spharm.laplacian_response(3, radius=1.0), [0, -2, -6, -12])
    rng = np.random.default_rng(3)
    for m, nn in ((0, 0), (0, 3), (2, 5), (8, 8)):
        c = np.zeros(S.packed_rows(T), dtype=np.complex128)
        c[spharm.packed_row(m, nn, T)] = 1.0 + (0.5j if m else 0.0)
        y = tr.synthesis(c)
        assert np.abs(tr.synthesis(c, lap) - (-nn * (nn + 1) / a ** 2) * y).max() <= 1e-12 * max(nn * (nn + 1), 1) / a ** 2
    c = S.random_packed(rng, T)
    x = tr.synthesis(c)
    back = tr.synthesis(tr.coefficients(tr.synthesis(c, lap)), inv)
    assert np.abs(back - (x - c[0].real)).max() <= 1e-10                   # the inverse undoes it apart from the mean a_0^0
    cut = tr.synthesis(c, spharm.truncation_response(T, 4))
    low = _transform(kind, nlat, L, 4)
    assert np.abs(cut - low.synthesis(low.coefficients(x))).max() <= 1e-11
    with pytest.raises(ValueError, match='response'):
        tr.synthesis(c, np.ones(T))
    with pytest.raises(ValueError, match='coefficients'):
        tr.synthesis(c[:-1])
    p32, p64 = tr.synthesis_tables()
    assert p32.dtype == np.float32 and p32.shape == (S.packed_rows(T), 20) and not p32[:, nlat:].any()
    assert np.array_equal(p32[:, :nlat], p64.astype(np.float32))
    assert np.abs(p64 * (0.5 * tr.weights) - tr.table64).max() <= 1e-15


def test_the_bounds_hold_for_a_sequential_fp32_evaluation():
    """the emulation of the kernels' scheme stays inside analysis_bound and synthesis_bound over the shapes of the GPU tests (two
    fields per shape: the field count does not enter the rounding)"""
    worst_a = worst_s = 0.0
    for n, (kind, nlat, L, T, _, _) in enumerate(S.grid_cases()):
        rng = np.random.default_rng(n)
        x = R.make_field(rng, (2, nlat, L), 'red' if n % 2 else 'white', 280.0 if n % 3 == 0 else 0.0)
        got = S.emulate_analysis(x, kind, T).astype(np.complex128)
        err = np.abs(got - S.analysis(x.astype(np.float64), kind, T)).max(axis=-1)
        lim = S.analysis_bound(x.astype(np.float64), kind)
        worst_a = max(worst_a, float((err / lim).max()))
        assert (err <= lim).all(), (kind, nlat, L, T)
        c = S.random_packed(rng, T, (2,), slope=(n % 3) * 0.5).astype(np.complex64)
        resp = [None, spharm.truncation_response(T, T // 2), spharm.laplacian_response(T, radius=1.0)][n % 3]
        r32 = None if resp is None else resp.astype(np.float32)
        y = S.emulate_synthesis(c, kind, nlat, L, r32)
        ref = S.synthesis(c, kind, nlat, L, None if r32 is None else r32.astype(np.float64))
        lim = S.synthesis_bound(c, kind, nlat, None if r32 is None else r32.astype(np.float64))[..., None]
        err = np.abs(y - ref)
        worst_s = max(worst_s, float((err / np.maximum(lim, np.finfo(np.float64).tiny)).max()))
        assert (err <= lim).all(), (kind, nlat, L, T)
    print('largest fraction of the bound: analysis %.4f, synthesis %.4f' % (worst_a, worst_s))
