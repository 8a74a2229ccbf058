"""
CPU tests of the spectra along time (DLWP.verify time_spectrum, time_cross_spectrum, time_coherence, time_fourier,
wavenumber_frequency_spectrum): the host path of every function against the reference of tests/time_spectrum_ref.py, the
travelling-wave and Parseval properties of the wavenumber-frequency spectrum, coherence, labels, argument errors, and the
host-only plan query of the device kernel.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import time_spectrum_ref as R    # noqa: E402

from DLWP import verify as V     # noqa: E402
from DLWP.model.extensions import Forecast  # noqa: E402


def _series(seed, T, shape, offset=0.0):
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    return R.make_series(rng, T, n, offset).reshape((T,) + tuple(shape))


@pytest.mark.parametrize('M,hop,kind,detrend,n_freq', ((8, None, 'hann', 'constant', None), (9, 3, 'boxcar', None, 2),
                                                       (32, 35, 'random', 'constant', 5), (5, 1, 'hann', None, None)))
def test_host_path_against_the_reference(M, hop, kind, detrend, n_freq):
    h = max(M // 2, 1) if hop is None else hop
    x = _series(M, R.rows_for(M, h), (2, 3), offset=0.25)
    y = _series(M + 1, x.shape[0], (2, 3))
    x[3, 0, 1] = np.nan
    y[x.shape[0] - 1, 1, 2] = -np.inf
    rng = np.random.default_rng(3)
    w = R.window(kind, M, rng)
    win = kind if kind != 'random' else w
    ref = R.reference(x.reshape(x.shape[0], -1), M, h, w, detrend is not None, n_freq, b=y.reshape(x.shape[0], -1))
    one = R.reference(x.reshape(x.shape[0], -1), M, h, w, detrend is not None, n_freq)
    K = R.clip_freq(n_freq, M)
    tol = dict(rtol=1e-6, atol=1e-9, equal_nan=True)           # (the host path subtracts the unrounded float64 mean)
    p, cnt = V.time_spectrum(x, M, hop=hop, window=win, detrend=detrend, n_freq=n_freq, return_count=True)
    assert p.shape == (K, 2, 3) and np.allclose(p.reshape(K, -1), one['power'][0], **tol)
    assert cnt.dtype == np.int32 and np.array_equal(cnt.reshape(-1), one['count'])
    cs, cnt = V.time_cross_spectrum(x, y, M, hop=hop, window=win, detrend=detrend, n_freq=n_freq, return_count=True)
    assert np.array_equal(cnt.reshape(-1), ref['count'])
    for i in range(4):
        assert np.allclose(cs[i].reshape(K, -1), ref['power'][i], **tol)
    coh = V.time_coherence(x, y, M, hop=hop, window=win, detrend=detrend, n_freq=n_freq)
    with np.errstate(invalid='ignore', divide='ignore'):
        want = (ref['power'][2] ** 2 + ref['power'][3] ** 2) / (ref['power'][0] * ref['power'][1])
    assert np.allclose(coh.reshape(K, -1), want, rtol=1e-5, atol=1e-9, equal_nan=True)
    z = V.time_fourier(x, n_segment=M, hop=hop, window=win, detrend=detrend, n_freq=n_freq)
    assert z.shape == (4, K, 2, 3) and z.dtype == np.complex128
    scale = np.nanmax(np.abs(one['coef'])) + 1.0
    assert np.allclose(z.reshape(4, K, -1), one['coef'], rtol=0, atol=1e-6 * scale, equal_nan=True)
    # min_count above what a column with a missing segment attains
    p3 = V.time_spectrum(x, M, hop=hop, window=win, detrend=detrend, n_freq=n_freq, min_count=4)
    assert np.array_equal(np.isnan(p3[0]).reshape(-1), one['count'] < 4)


def test_other_axis_and_whole_series_fourier():
    x = _series(1, 40, (3,))
    a = V.time_spectrum(x, 16, hop=8)
    b = V.time_spectrum(np.ascontiguousarray(x.T), 16, axis=1, hop=8)
    assert b.shape == (3, 9) and np.allclose(a, b.T, rtol=1e-12)
    z = V.time_fourier(x)
    assert z.shape == (21, 3) and np.allclose(z, np.fft.rfft(x.astype(np.float64), axis=0), atol=1e-9)
    short = V.time_spectrum(x[:10], 16, return_count=True)
    assert np.isnan(short[0]).all() and short[0].shape == (9, 3) and np.array_equal(short[1], np.zeros(3, np.int32))
    assert V.time_fourier(x[:10], n_segment=16).shape == (0, 9, 3)
    one = V.time_spectrum(x[:16], 16, return_count=True)
    assert np.isfinite(one[0]).all() and np.array_equal(one[1], np.ones(3, np.int32))


def test_spectral_window():
    assert np.array_equal(V.spectral_window('boxcar', 5), np.ones(5))
    h = V.spectral_window('hann', 8)
    assert h[0] == 0.0 and np.isclose(h[4], 1.0) and np.allclose(h[:4] + h[4:], 1.0)           # periodic: overlaps to a constant
    w = np.arange(4.0)
    assert np.array_equal(V.spectral_window(w, 4), w)
    with pytest.raises(ValueError):
        V.spectral_window(w, 5)
    with pytest.raises(ValueError):
        V.spectral_window('hamming', 4)


def test_coherence_of_related_and_unrelated_series():
    a = _series(7, 16 * 65, (6,))
    assert np.allclose(V.time_coherence(a, 2.0 * a, 32), 1.0, rtol=1e-9)
    b = _series(8, 16 * 65, (6,))
    coh, cnt = V.time_coherence(a, b, 32, hop=32, window='boxcar', return_count=True)
    n_seg = 16 * 65 // 32
    assert np.all(cnt == n_seg)
    assert np.isnan(coh[0]).all()                                   # the mean was removed: no power at f = 0 on either side
    assert 0.4 / n_seg < coh[1:].mean() < 2.5 / n_seg                                         # about 1 / n_seg
    zero = V.time_coherence(a, np.zeros_like(a), 32, detrend=None)
    assert np.isnan(zero).all()


@pytest.mark.parametrize('M,L,k0,f0', ((32, 16, 3, 5), (30, 9, 2, 7), (16, 8, 4, 3), (16, 8, 1, 8), (16, 8, 2, 0)))
def test_travelling_wave_lands_in_one_bin(M, L, k0, f0):
    T = 3 * M
    t = np.arange(T)[:, None, None]
    lon = 2.0 * np.pi * np.arange(L)[None, None, :] / L
    lat = np.array([0.5, 1.0, 2.0])[None, :, None]
    x = lat * np.cos(k0 * lon - 2.0 * np.pi * f0 * t / M)
    r = V.wavenumber_frequency_spectrum(x, M, window='boxcar', detrend=None, hop=M)
    assert r.eastward.shape == (M // 2 + 1, 3, L // 2 + 1)
    total = r.eastward.sum(axis=(0, 2)) + r.westward.sum(axis=(0, 2))
    assert np.allclose(total, (x ** 2).mean(axis=(0, 2)), rtol=1e-10)
    stand = f0 == 0 or 2 * f0 == M or 2 * k0 == L                  # f = 0, Nyquist in time or in longitude: half in each
    e, w = r.eastward[f0, :, k0], r.westward[f0, :, k0]
    if stand:
        assert np.allclose(e, w, rtol=1e-9) and np.allclose(e + w, total, rtol=1e-9)
    else:
        assert np.allclose(e, total, rtol=1e-9) and np.all(np.abs(w) <= 1e-12 * total)
        back = V.wavenumber_frequency_spectrum(x[::-1], M, window='boxcar', detrend=None, hop=M)
        assert np.allclose(back.westward[f0, :, k0], total, rtol=1e-9)
    rest = r.eastward.copy()
    rest[f0, :, k0] = 0.0
    assert np.all(np.abs(rest) <= 1e-12 * total[None, :, None])


def test_wavenumber_frequency_parseval_components_and_labels():
    M, hop, L = 16, 8, 12
    x = _series(2, 40, (4, L), offset=0.5).astype(np.float64)
    r, cnt = V.wavenumber_frequency_spectrum(x, M, hop=hop, return_count=True)
    w = V.spectral_window('hann', M).astype(np.float32).astype(np.float64)
    want = np.zeros(4)
    for s in range(4):
        seg = x[s * hop:s * hop + M]
        zk = np.fft.rfft(seg, axis=-1)                              # detrending acts per wavenumber: on the zonal coefficients
        zk = zk - zk.mean(axis=0)
        y = np.fft.irfft(zk, n=L, axis=-1) * w[:, None, None]
        want += (y ** 2).sum(axis=0).mean(axis=-1) / (w ** 2).sum()
    assert np.allclose(r.eastward.sum(axis=(0, 2)) + r.westward.sum(axis=(0, 2)), want / 4, rtol=1e-10)
    assert cnt.shape == (4, L // 2 + 1) and np.all(cnt == 4)
    sym = V.wavenumber_frequency_spectrum(x, M, hop=hop, lat_axis=1, component='symmetric')
    anti = V.wavenumber_frequency_spectrum(x, M, hop=hop, lat_axis=1, component='antisymmetric')
    assert np.allclose(sym.eastward, sym.eastward[:, ::-1]) and np.allclose(anti.westward, anti.westward[:, ::-1])
    both = V.wavenumber_frequency_spectrum((x + x[:, ::-1]) / 2, M, hop=hop)
    assert np.allclose(sym.eastward, both.eastward, rtol=1e-12)
    few = V.wavenumber_frequency_spectrum(x, M, hop=hop, n_wave=3, n_freq=4)
    assert few.westward.shape == (4, 4, 3) and np.allclose(few.westward, r.westward[:4, :, :3], rtol=1e-12)
    # a row with a hole: its latitude loses the segments that hold the row
    x[9, 2, 5] = np.nan
    r2, c2 = V.wavenumber_frequency_spectrum(x, M, hop=hop, return_count=True)
    assert np.all(c2[2] == 2) and np.all(c2[[0, 1, 3]] == 4) and np.isfinite(r2.eastward).all()
    lat = np.array([-30., -10., 10., 30.])
    fc = Forecast(x, ('time', 'lat', 'lon'), {'time': np.arange(40), 'lat': lat, 'lon': np.arange(L) * 30.})
    lab, lc = V.wavenumber_frequency_spectrum(fc, M, hop=hop, component='symmetric', return_count=True)
    assert lab.eastward.dims == ('frequency', 'lat', 'wavenumber') and lc.dims == ('lat', 'wavenumber')
    assert np.array_equal(lab.eastward.coords['frequency'], np.arange(9) / 16.) and np.array_equal(lab.westward.coords['lat'], lat)
    assert np.array_equal(lab.eastward.coords['wavenumber'], np.arange(7))
    bad = Forecast(x, ('time', 'lat', 'lon'), {'lat': np.array([-30., -10., 10., 35.])})
    with pytest.raises(ValueError):
        V.wavenumber_frequency_spectrum(bad, M, component='symmetric')


def test_labels_and_coordinates():
    x = _series(4, 48, (2, 3))
    fc = Forecast(x.transpose(1, 0, 2), ('lat', 'time', 'lon'), {'time': np.arange(48) * 6, 'lat': np.array([1., 2.]),
                                                                 'lon': np.array([0., 120., 240.])})
    p, cnt = V.time_spectrum(fc, 16, return_count=True)
    assert p.dims == ('lat', 'frequency', 'lon') and p.values.shape == (2, 9, 3) and cnt.dims == ('lat', 'lon')
    assert np.array_equal(p.coords['frequency'], np.arange(9) / 16.) and np.array_equal(p.coords['lon'], fc.coords['lon'])
    assert 'time' not in p.coords and np.allclose(p.values, V.time_spectrum(x, 16).transpose(1, 0, 2))
    cs = V.time_cross_spectrum(fc, fc, 16, n_freq=4)
    assert cs._fields == ('power_a', 'power_b', 'co', 'quad') and cs.co.dims == p.dims and cs.quad.values.shape == (2, 4, 3)
    z = V.time_fourier(fc, n_segment=16)
    assert z.dims == ('segment', 'lat', 'frequency', 'lon') and z.values.shape == (5, 2, 9, 3)
    assert V.time_fourier(fc, axis='time').dims == ('lat', 'frequency', 'lon')
    assert V.time_coherence(fc, fc, 16).name == 'time_coherence'
    other = Forecast(fc.values, fc.dims, dict(fc.coords, lon=np.array([0., 100., 240.])))
    with pytest.raises(ValueError):
        V.time_cross_spectrum(fc, other, 16)


def test_argument_errors():
    x = _series(5, 40, (3,))
    for kw in (dict(n_segment=1), dict(n_segment=16, hop=0), dict(n_segment=16, n_freq=10), dict(n_segment=16, n_freq=0),
               dict(n_segment=16, min_count=0), dict(n_segment=16, detrend='linear'), dict(n_segment=16, window='hamming'),
               dict(n_segment=16, window=np.ones(15)), dict(n_segment=16, window=np.zeros(16)), dict(n_segment=16, axis=2)):
        with pytest.raises(ValueError):
            V.time_spectrum(x, **kw)
    with pytest.raises(ValueError):
        V.time_cross_spectrum(x, x[:, :2], 16)
    with pytest.raises(ValueError):
        V.wavenumber_frequency_spectrum(x, 16, lon_axis=0)
    with pytest.raises(ValueError):
        V.wavenumber_frequency_spectrum(x, 16, n_wave=3)
    with pytest.raises(ValueError):
        V.wavenumber_frequency_spectrum(x, 16, component='symmetric')
    with pytest.raises(ValueError):
        V.wavenumber_frequency_spectrum(x, 16, lat_axis=1, component='even')


def test_plan_query():
    """the host-only plan query of dlwpcs_time_spectrum: tile counts, the split choice, the vector flag, the limits"""
    from DLWP import ops
    from DLWP import _native as nat
    p = ops.time_spectrum_plan((4096, 65536), (65536, 1), 512, hop=256)
    assert p['n_seg'] == 15 and p['col_tiles'] == 2048 and p['freq_tiles'] == 3 and p['slabs'] == 2
    assert not p['split'] and p['tiles'] == 2048 * 3 and p['grid'] == 512 and p['vec'] and 0 < p['lds_bytes'] <= 64 << 10
    assert not ops.time_spectrum_plan((4096, 65536), (65536, 1), 512, hop=256, aligned=False)['vec']
    assert not ops.time_spectrum_plan((4096, 65534), (65534, 1), 512)['vec']
    few = ops.time_spectrum_plan((4096, 40), (40, 1), 64, hop=32, n_freq=33)
    assert few['n_seg'] == 127 and few['slabs'] == 16 and few['split'] and few['tiles'] == 2 * 1 * 16 and few['grid'] == 32
    assert not ops.time_spectrum_plan((4096, 40), (40, 1), 64, hop=32, split=False)['split']
    assert ops.time_spectrum_plan((4096, 65536), (65536, 1), 512, hop=256, split=True)['tiles'] == 2048 * 3 * 2
    one = ops.time_spectrum_plan((70, 40), (40, 1), 64, hop=32, split=True)
    assert one['n_seg'] == 1 and not one['split'] and one['tiles'] == 2                      # one slab: nothing to add up
    none = ops.time_spectrum_plan((10, 40), (40, 1), 64, pair=True)
    assert none['n_seg'] == 0 and none['slabs'] == 0 and none['tiles'] == 2                  # NaN is still written
    coef = ops.time_spectrum_plan((1000, 40), (40, 1), 64, hop=4, coefficients=True)
    assert coef['n_seg'] == 235 and coef['tiles'] == 2 * 30 and ops.time_spectrum_plan((10, 40), (40, 1), 64, coefficients=True)['tiles'] == 0
    big = ops.time_spectrum_plan((2, 65537 * 32 + 5), (65537 * 32 + 5, 1), 2)
    assert big['col_tiles'] == 65538 and big['tiles'] == 65538 > 65536 and big['grid'] == 512
    zonal = ops.time_spectrum_plan((30, 144), (144, 1), 144, row_axis=1, coefficients=True)
    assert zonal['n_seg'] == 1 and zonal['col_tiles'] == 1 and not zonal['vec']
    assert ops.time_spectrum_plan((1728, 8), (8, 1), 1728)['n_seg'] == 1
    with pytest.raises(NotImplementedError):
        ops.time_spectrum_plan((4000, 8), (8, 1), 1729)
    d, _ = ops.rows_layout((4000, 8), (8, 1), 0, None, 4)
    import ctypes
    info = (ctypes.c_int64 * 8)()
    rc = nat.lib().dlwpcs_time_spectrum_plan_info(ctypes.byref(d), 1 << 20, None, 4000, 1729, 1, 0, 0, -1, info)
    assert rc == nat.lib().dlwpcs_time_spectrum_plan_info(ctypes.byref(d), 1 << 20, None, 4000, 4000, 1, 0, 0, -1, info) != 0
    with pytest.raises(NotImplementedError):
        nat.check(rc, 'dlwpcs_time_spectrum_plan_info')
    for args in ((4000, 1, 1, 0, 0, -1), (4000, 8, 0, 0, 0, -1), (4000, 8, 1, 6, 0, -1), (4000, 8, 1, 0, 2, -1), (4000, 8, 1, 0, 0, 2),
                 (-1, 8, 1, 0, 0, -1)):
        rc = nat.lib().dlwpcs_time_spectrum_plan_info(ctypes.byref(d), 1 << 20, None, args[0], args[1], args[2], args[3], args[4], args[5], info)
        with pytest.raises(ValueError):
            nat.check(rc, 'dlwpcs_time_spectrum_plan_info')
    assert nat.lib().dlwpcs_time_spectrum_plan_info(ctypes.byref(d), None, None, 4000, 8, 4, 0, 0, -1, info) != 0      # null source
    assert nat.lib().dlwpcs_time_spectrum_scratch_bytes(ctypes.byref(d), 4000, 8, 4, 0, 1, 1) == 125 * 4 * 5 * 8 * 8 + 125 * 8 * 4
    assert nat.lib().dlwpcs_time_spectrum_scratch_bytes(ctypes.byref(d), 4000, 8, 4, 0, 0, 0) == 0
