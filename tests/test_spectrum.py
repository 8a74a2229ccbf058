"""
Zonal spectra on the host (DLWP.verify.zonal_spectrum, zonal_cross_spectrum, zonal_coherence with numpy inputs) against the
float64 reference of spectrum_ref.py and against first principles, and the descriptor DLWP.ops builds for the device kernel,
checked in pure Python against a brute-force enumeration of every row's offset.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import spectrum_ref as R     # noqa: E402

from DLWP import verify      # noqa: E402
from DLWP.model.extensions import Forecast     # noqa: E402

HOST_L = [2, 3, 4, 5, 8, 9, 12, 45, 360]


@pytest.mark.parametrize('L', HOST_L)
def test_parseval_and_reference(L):
    rng = np.random.default_rng(L)
    x = rng.standard_normal((3, 7, L)) + 2.5
    p = verify.zonal_spectrum(x, axis=())
    assert p.shape == (3, 7, L // 2 + 1) and p.dtype == np.float64
    ms = (x ** 2).mean(axis=-1)
    assert np.abs(p.sum(axis=-1) - ms).max() <= 1e-12 * ms.max()
    ref, _, _ = R.reference(x, None, ())
    assert np.abs(p - ref[0]).max() <= 1e-12 * ms.max()
    for c in R.grid_cases(L)[::3]:
        f = R.make_field(rng, (c['groups'], c['rows'], L), c['kind'])
        v = R.make_field(rng, (c['groups'], c['rows'], L)) if c['pair'] else None
        w = R.make_weights(c['weights'], rng, c['groups'], c['rows'])
        ref, _, m = R.reference(f, v, (1,), w, c['n_wave'], c['remove_mean'])
        if c['pair']:
            got = np.stack(verify.zonal_cross_spectrum(f, v, axis=1, weights=w, n_wave=c['n_wave'], remove_mean=c['remove_mean']))
        else:
            got = verify.zonal_spectrum(f, axis=1, weights=w, n_wave=c['n_wave'], remove_mean=c['remove_mean'])[None]
        assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref))
        ok = ~np.isnan(ref)
        assert (np.abs(got - ref)[ok] <= 1e-12 * np.nanmax(m)).all()


@pytest.mark.parametrize('L', [8, 9, 12, 45])
def test_pure_tones(L):
    j = np.arange(L)
    for k0 in range(L // 2 + 1):
        for phi in (0.0, 0.7):
            x = np.cos(2 * np.pi * k0 * j / L + phi)
            p = verify.zonal_spectrum(x)
            if k0 == 0 or 2 * k0 == L:
                want = np.cos(phi) ** 2                  # c_k = 1: the tone is cos(phi) (-1)^j or cos(phi) itself
            else:
                want = 0.5
            assert abs(p[k0] - want) <= 1e-14
            rest = np.delete(p, k0)
            assert rest.size == 0 or rest.max() <= 1e-20


def test_n_wave_and_remove_mean():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((4, 6, 45)) + 280.0
    full = verify.zonal_spectrum(x, axis=1)
    for n in (1, 2, 23):
        assert np.array_equal(verify.zonal_spectrum(x, axis=1, n_wave=n), full[..., :n])
    rm = verify.zonal_spectrum(x, axis=1, remove_mean=True)
    assert np.abs(rm[..., 1:] - full[..., 1:]).max() <= 1e-9             # (the offset's rounding, 280^2 * 2^-52 * L)
    assert np.abs(rm[..., 0] - full[..., 0]).max() <= 1e-12 * 280.0 ** 2
    assert np.abs(rm[..., 0] - (x.mean(axis=-1) ** 2).mean(axis=1)).max() <= 1e-12 * 280.0 ** 2


def test_missing_rows_are_left_out_and_counted():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((3, 6, 12))
    y = x.copy()
    y[0, 0, 3] = np.nan
    y[0, 5, 11] = np.inf
    y[1, :, 0] = -np.inf
    p, n = verify.zonal_spectrum(y, axis=1, return_count=True)
    assert n.tolist() == [2, 6, 0] and n.dtype == np.int32
    assert np.isnan(p[1]).all()
    assert np.array_equal(p[0], verify.zonal_spectrum(x[0, 1:5], axis=0)) and np.array_equal(p[2], verify.zonal_spectrum(x[2], axis=0))
    # the pair form: a row counts only when both rows are finite
    v = x[:, ::-1].copy()
    v[2, 1, 0] = np.nan
    c, n = verify.zonal_cross_spectrum(y, v, axis=1, return_count=True)
    assert n.tolist() == [2, 6, 1]
    keep = [0, 2, 3, 4, 5]
    assert np.allclose(c.power_f[2], verify.zonal_spectrum(x[2, keep], axis=0), rtol=1e-14, atol=0)


def test_weights_zero_band_and_cos_lat():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((4, 9, 16))
    band = np.zeros(9)
    band[2:5] = 1.0
    assert np.allclose(verify.zonal_spectrum(x, axis=1, weights=band), verify.zonal_spectrum(x[:, 2:5], axis=1), rtol=1e-13)
    assert np.isnan(verify.zonal_spectrum(x, axis=1, weights=np.zeros(9))).all()
    lat = np.linspace(-80, 80, 9)
    fx = Forecast(x, ('time', 'lat', 'lon'), {'time': np.arange(4), 'lat': lat, 'lon': np.arange(16) * 22.5})
    fx.lat = Forecast(lat, ('lat',), {'lat': lat})
    cw = np.cos(np.deg2rad(lat))
    p = verify.zonal_spectrum(fx, axis='lat', weighted=True, weights=band)
    want = (verify.zonal_spectrum(x, axis=()) * (cw * band)[None, :, None]).sum(axis=1) / (cw * band).sum()
    assert isinstance(p, Forecast) and p.dims == ('time', 'wavenumber')
    assert np.array_equal(p.coords['wavenumber'], np.arange(9)) and np.array_equal(p.coords['time'], np.arange(4))
    assert np.allclose(p.values, want, rtol=1e-13)
    with pytest.raises(ValueError):
        verify.zonal_spectrum(x, axis=1, weights=np.ones(8))
    with pytest.raises(ValueError):
        verify.zonal_spectrum(x, axis=1, weights=np.full(9, np.nan))


def test_kept_and_averaged_axes_in_any_order():
    rng = np.random.default_rng(6)
    x = rng.standard_normal((3, 5, 2, 7, 12))
    rows = verify.zonal_spectrum(x, axis=())
    for ax in [(0,), (1, 3), (3, 1), (0, 1, 2, 3), (2,), (-2, 0)]:
        got = verify.zonal_spectrum(x, axis=ax)
        assert np.allclose(got, rows.mean(axis=tuple(a % 5 for a in ax)), rtol=1e-13)
    assert np.allclose(verify.zonal_spectrum(x), rows.mean(axis=(0, 1, 2, 3)), rtol=1e-13)
    moved = np.moveaxis(x, -1, 1)                                        # longitude on axis 1
    assert np.allclose(verify.zonal_spectrum(moved, lon_axis=1, axis=(0, 3)), rows.mean(axis=(0, 2)), rtol=1e-13)
    with pytest.raises(ValueError):
        verify.zonal_spectrum(x, axis=(4,))


def test_labelled_inputs_find_lon_by_name():
    rng = np.random.default_rng(7)
    x = rng.standard_normal((3, 8, 4))
    fx = Forecast(x, ('f_hour', 'lon', 'lat'), {'f_hour': np.array([6, 12, 18]), 'lon': np.arange(8) * 45., 'lat': np.arange(4) * 10.})
    p = verify.zonal_spectrum(fx, axis='lat')
    assert p.dims == ('f_hour', 'wavenumber') and np.array_equal(p.coords['f_hour'], [6, 12, 18])
    assert np.allclose(p.values, verify.zonal_spectrum(x, lon_axis=1, axis=2), rtol=1e-14)
    other = Forecast(x, ('f_hour', 'lon', 'lat'), {'f_hour': np.array([6, 12, 24]), 'lon': fx.coords['lon'], 'lat': fx.coords['lat']})
    with pytest.raises(ValueError):
        verify.zonal_coherence(fx, other)
    c = verify.zonal_cross_spectrum(fx, fx, axis='lat')
    assert c.co.dims == ('f_hour', 'wavenumber') and c._fields == ('power_f', 'power_v', 'co', 'quad')


def test_pair_form_identity_shift_and_noise():
    rng = np.random.default_rng(8)
    L, rows = 24, 400
    f = rng.standard_normal((rows, L))
    c = verify.zonal_cross_spectrum(f, f)
    assert np.array_equal(c.power_f, c.power_v) and np.abs(c.quad).max() <= 1e-16 and np.allclose(c.co, c.power_f, rtol=1e-14)
    assert np.abs(verify.zonal_coherence(f, f) - 1).max() <= 1e-12
    s = 5
    c = verify.zonal_cross_spectrum(f, np.roll(f, s, axis=-1))
    k = np.arange(L // 2 + 1)
    want = np.exp(2j * np.pi * k * s / L)
    got = (c.co + 1j * c.quad) / c.power_f
    inner = slice(1, L // 2)                                             # (k = 0 and Nyquist are real: the phase folds)
    assert np.abs(got[inner] - want[inner]).max() <= 1e-12
    assert np.abs(verify.zonal_coherence(f, np.roll(f, s, axis=-1))[inner] - 1).max() <= 1e-12
    g = rng.standard_normal((rows, L))
    assert verify.zonal_coherence(f, g).max() <= 10.0 / rows
    per_row = verify.zonal_coherence(f, g, axis=())
    assert np.abs(per_row[:, inner] - 1).max() <= 1e-9                   # why coherence is formed from the averages


def test_refusals():
    x = np.zeros((3, 4, 8))
    with pytest.raises(NotImplementedError, match='aligned'):
        verify.zonal_cross_spectrum(x, x[0])
    with pytest.raises(NotImplementedError, match='aligned'):
        verify.zonal_coherence(x, x[0])
    for bad in (0, 6, -1):
        with pytest.raises(ValueError):
            verify.zonal_spectrum(x, n_wave=bad)
    with pytest.raises(ValueError):
        verify.zonal_spectrum(np.zeros((3, 1)))
    with pytest.raises(ValueError):
        verify.zonal_cross_spectrum(x, np.zeros((3, 4, 9)))
    with pytest.raises(ValueError):
        verify.zonal_spectrum(x, lon_axis=3)
    with pytest.raises(ValueError):
        verify.zonal_spectrum(x, axis=(1, 1))


def test_device_functions_refuse_host_tensors():
    import torch
    from DLWP import _native as nat, ops
    with pytest.raises(nat.NativeError):
        ops.zonal_spectrum(torch.zeros((3, 8)))


SHAPES = [((3, 5, 2, 7), {1, 3}), ((3, 5, 2, 7), {0, 1}), ((3, 5, 2, 7), set()), ((3, 5, 2, 7), {0, 1, 2, 3}), ((1, 5, 1, 7), {1}),
          ((4, 6), {0}), ((), set()), ((70, 1, 33), {2})]


@pytest.mark.parametrize('shape,reduced', SHAPES)
def test_descriptor_for_contiguous_permuted_and_strided_inputs(shape, reduced):
    from DLWP import _native as nat, ops
    L = 12
    nd = len(shape)
    contiguous = tuple(int(np.prod(shape[i + 1:], dtype=np.int64)) * L for i in range(nd))
    permuted = [0] * nd                                                  # a permuted view: the axes stored in reverse order
    acc = L
    for i in range(nd):
        permuted[i] = acc
        acc *= shape[i]
    strided = tuple(2 * s + (4 if i == 0 else 0) for i, s in enumerate(contiguous))    # every other row, padded planes
    wts = tuple(0 if i % 2 == 0 else int(np.prod([shape[j] for j in range(i + 1, nd) if j % 2], dtype=np.int64))
                for i in range(nd))                                      # weights broadcast along the even axes
    for a_st, b_st in ((contiguous, contiguous), (tuple(permuted), contiguous), (strided, tuple(permuted))):
        strides = [a_st, b_st, wts]
        dims = ops.spectrum_dims(shape, strides, reduced)
        assert len(dims) <= nd and all(e > 1 for e, _, _ in dims)
        want = R.spectrum_dims_reference(shape, strides, reduced)
        got = R.dims_offsets(dims, 3)
        assert got.shape == want.shape and np.array_equal(got, want)
        d = ops.spectrum_desc(L, dims, n_wave=3, remove_mean=True)
        assert (d.L, d.n_wave, d.n_dims, d.remove_mean) == (L, 3, len(dims), 1)
        for i, (e, st, kept) in enumerate(dims):
            assert d.ext[i] == e and d.kept[i] == int(kept) and [d.stride[k][i] for k in range(3)] == list(st)
    if shape == (3, 5, 2, 7) and reduced == {0, 1}:                      # contiguous neighbours with one flag merge
        assert ops.spectrum_dims(shape, [contiguous] * 3, reduced) == [(15, (14 * L,) * 3, False), (14, (L,) * 3, True)]
    assert isinstance(ops.spectrum_desc(L, []), nat.ZonalSpectrumDesc)


def test_twiddle_table_is_correctly_rounded():
    from DLWP import ops
    for L in (2, 3, 8, 45, 1440):
        t = ops.spectrum_twiddle_host(L)
        assert t.shape == (L, 2) and t.dtype == np.float32
        m = np.arange(L)
        exact = np.stack([np.cos(2 * np.pi * m / L), -np.sin(2 * np.pi * m / L)], axis=1)
        assert np.abs(t.astype(np.float64) - exact).max() <= 2.0 ** -25 + 1e-15
        assert t[0, 0] == 1.0 and abs(t[0, 1]) == 0.0
