"""
Spherical-harmonic spectra on the host (DLWP.verify.spherical_spectrum, spherical_cross_spectrum, spherical_correlation with numpy
and labelled inputs) against the float64 reference of sht_ref.py, their refusals, and the host-side validation of the device entry
points through ctypes (descriptor errors are caught before any launch: no device is needed).
"""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sht_ref as R     # noqa: E402

from DLWP import verify      # noqa: E402
from DLWP.model.extensions import Forecast     # noqa: E402

KIND, NLAT, L, T = 'clenshaw-curtis', 17, 36, 8
LAT = R.latitudes(KIND, NLAT)


def test_host_path_against_the_reference_and_axis_handling():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((3, 4, NLAT, L)) + 2.0
    y = rng.standard_normal((3, 4, NLAT, L))
    rows = verify.spherical_spectrum(x, lat=LAT, axis=())
    assert rows.shape == (3, 4, T + 1) and rows.dtype == np.float64
    ref, _, _ = R.reference(x, None, KIND, T)
    assert np.abs(rows - ref[0]).max() <= 1e-13 * np.abs(ref).max()
    for axis, red in ((None, (0, 1)), (0, (0,)), (1, (1,)), ((0, 1), (0, 1)), (-3, (1,))):
        got = verify.spherical_spectrum(x, lat=LAT, axis=axis)
        want, _, _ = R.reference(x, None, KIND, T, red)
        assert got.shape == want.shape[1:] and np.abs(got - want[0]).max() <= 1e-13 * np.abs(want).max()
    # a smaller truncation is the head of the larger one; the default is the largest the grid allows
    assert np.abs(verify.spherical_spectrum(x, lat=LAT, axis=(), truncation=5) - rows[..., :6]).max() <= 1e-14
    # grid axes anywhere, latitudes in either direction
    xt = np.ascontiguousarray(x.transpose(2, 0, 3, 1)[::-1])
    got = verify.spherical_spectrum(xt, lat=LAT[::-1], lat_axis=0, lon_axis=2, axis=())
    assert np.abs(got - rows).max() <= 1e-13 * np.abs(rows).max()
    # the pair form, and the correlation from the averaged quantities
    cs = verify.spherical_cross_spectrum(x, y, lat=LAT, axis=0)
    ref, _, _ = R.reference(x, y, KIND, T, (0,))
    assert cs._fields == ('power_f', 'power_v', 'co')
    assert np.abs(np.stack(cs) - ref).max() <= 1e-13 * np.abs(ref).max()
    cor = verify.spherical_correlation(x, y, lat=LAT, axis=0)
    assert np.abs(cor - ref[2] / np.sqrt(ref[0] * ref[1])).max() <= 1e-12 and (np.abs(cor) <= 1 + 1e-12).all()
    assert np.abs(verify.spherical_correlation(x, 3.0 * x, lat=LAT) - 1.0).max() <= 1e-12
    # Parseval for a band-limited field, and S_0 the squared global mean
    a = R.random_coefficients(rng, T)
    z = R.synthesis(a, KIND, NLAT, L)
    S = verify.spherical_spectrum(z, lat=LAT)
    assert S.shape == (T + 1,) and abs(S.sum() - R.mean_square(z, KIND)) <= 1e-12 * S.sum() and abs(S[0] - a[0, 0].real ** 2) <= 1e-12


def test_labelled_inputs_find_the_grid_by_name_and_carry_degree():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((3, L, NLAT, 2))
    coords = {'f_hour': np.array([6, 12, 18]), 'lon': np.arange(L) * 10., 'lat': LAT, 'varlev': np.array(['z', 't'])}
    fx = Forecast(x, ('f_hour', 'lon', 'lat', 'varlev'), coords)
    got = verify.spherical_spectrum(fx, axis='varlev')
    assert got.dims == ('f_hour', 'degree') and np.array_equal(got.coords['degree'], np.arange(T + 1))
    assert np.array_equal(got.coords['f_hour'], coords['f_hour'])
    want = verify.spherical_spectrum(x, lat=LAT, lat_axis=2, lon_axis=1, axis=3)
    assert np.array_equal(got.values, want)
    cs = verify.spherical_cross_spectrum(fx, fx, axis=())
    assert cs.co.dims == ('f_hour', 'varlev', 'degree') and np.allclose(cs.co.values, cs.power_f.values, rtol=1e-13, atol=0)
    assert verify.spherical_correlation(fx, fx).dims == ('degree',)
    with pytest.raises(ValueError, match='averaged'):
        verify.spherical_spectrum(fx, axis='lat')


def test_missing_fields_are_left_out_and_counted():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((3, 5, NLAT, L))
    y = x.copy()
    y[0, 1, 3, 4] = np.nan
    y[0, 4, 0, 0] = np.inf
    y[2, :, 5, 5] = -np.inf
    got, cnt = verify.spherical_spectrum(y, lat=LAT, axis=1, return_count=True)
    assert cnt.dtype == np.int32 and cnt.tolist() == [2, 0, 5]
    assert np.isnan(got[2]).all() and not np.isnan(got[:2]).any()
    want = verify.spherical_spectrum(x[0, [0, 2, 3]], lat=LAT)
    assert np.abs(got[0] - want).max() <= 1e-14 * want.max()
    assert np.array_equal(got[1], verify.spherical_spectrum(x[1], lat=LAT))
    # the pair form counts a field only when it is finite in both; without return_count the result alone comes back
    cs, cnt2 = verify.spherical_cross_spectrum(x, y, lat=LAT, axis=1, return_count=True)
    assert cnt2.tolist() == [2, 0, 5] and np.abs(cs.power_f[0] - want).max() <= 1e-14 * want.max()
    assert isinstance(verify.spherical_spectrum(y, lat=LAT, axis=1), np.ndarray)
    rows, each = verify.spherical_spectrum(y, lat=LAT, axis=(), return_count=True)
    assert each.shape == (3, 5) and each.sum() == 7 and np.isnan(rows[0, 1]).all()


def test_refusals():
    from DLWP.remap import spharm
    x = np.zeros((3, NLAT, L))
    with pytest.raises(ValueError, match='neither'):                    # none of the three layouts
        verify.spherical_spectrum(x, lat=np.linspace(-80., 80., NLAT))
    with pytest.raises(ValueError, match='neither'):
        verify.spherical_spectrum(x, lat=np.concatenate([LAT[:-1], [-89.0]]))
    with pytest.raises(ValueError, match='above'):                      # the quadrature's limit: 2 T <= nlat - 1
        verify.spherical_spectrum(x, lat=LAT, truncation=T + 1)
    with pytest.raises(ValueError, match='longitudes'):                 # L >= 2 T + 1
        verify.spherical_spectrum(x[..., :16], lat=LAT, truncation=8)
    assert verify.spherical_spectrum(x[..., :16], lat=LAT).shape == (8,)        # None: the largest allowed, here (16 - 1) // 2
    with pytest.raises(ValueError, match='above'):
        spharm.SphericalTransform(R.latitudes('gauss', 8), 64, 8)
    assert spharm.SphericalTransform(R.latitudes('gauss', 8), 64, 7).truncation == 7
    with pytest.raises(NotImplementedError, match='aligned'):           # the lagged continuous-series form
        verify.spherical_cross_spectrum(np.zeros((2, 3, NLAT, L)), x, lat=LAT)
    with pytest.raises(ValueError, match='one shape'):
        verify.spherical_cross_spectrum(x, x[:2], lat=LAT)
    with pytest.raises(ValueError, match='latitudes'):
        verify.spherical_spectrum(x)                                    # unlabelled and no lat=
    with pytest.raises(ValueError, match='latitudes'):
        verify.spherical_spectrum(x, lat=LAT[:-1])
    with pytest.raises(TypeError):
        verify.spherical_spectrum(x, lat=LAT, weighted=True)            # the area weighting is inside the transform


def test_device_function_refuses_host_tensors():
    import torch
    from DLWP import _native as nat, ops
    from DLWP.remap import spharm
    tr = spharm.SphericalTransform(LAT, L)
    with pytest.raises(nat.NativeError):
        ops.spherical_spectrum(torch.zeros((3, NLAT, L)), transform=tr)


def _desc(nlat=NLAT, n_lon=L, trunc=T, fields=3):
    from DLWP import ops
    dims = ops.spectrum_dims((fields,), [(nlat * n_lon,), (nlat * n_lon,)], ())
    return ops.sht_desc(nlat, n_lon, trunc, dims, (n_lon, n_lon))


def test_descriptor_validation_on_the_host():
    """every descriptor error comes back before a launch with a message: fake (never dereferenced) device addresses suffice"""
    from DLWP import _native as nat
    lib = nat.lib()
    d = _desc()
    assert (d.nlat, d.L, d.T, d.n_dims, d.ext[0], d.stride[0][0], d.lat_stride[1]) == (NLAT, L, T, 1, 3, NLAT * L, L)
    nlp = (NLAT + 3) // 4 * 4
    assert lib.dlwpcs_sht_spectrum_scratch_bytes(ctypes.byref(d)) == 2 * 3 * (T + 1) * 2 * nlp * 4 + 3 * NLAT * 4
    A, TW, TAB, OUT, SCR = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000

    def call(desc, a=A, b=None, tw=TW, tab=TAB, scr=SCR, out=OUT):
        return lib.dlwpcs_sht_spectrum(ctypes.byref(desc), a, b, tw, tab, scr, out, None, None)

    for bad, word in ((_desc(trunc=18), b'truncation'), (_desc(trunc=-1), b'truncation'), (_desc(n_lon=1, trunc=0), b'longitudes'),
                      (_desc(nlat=1, trunc=0), b'latitudes')):
        assert call(bad) == -1 and word in lib.dlwpcs_last_error()
        assert lib.dlwpcs_sht_spectrum_scratch_bytes(ctypes.byref(bad)) == 0
    for bad in (_desc(n_lon=1730), _desc(nlat=nat.SHT_MAX_NLAT + 1)):
        assert call(bad) == -2 and b'serves' in lib.dlwpcs_last_error()
    with pytest.raises(NotImplementedError):
        nat.check(call(_desc(n_lon=1730)), 'dlwpcs_sht_spectrum')
    assert call(d, tab=None) == -1 and b'null' in lib.dlwpcs_last_error()
    assert call(d, tw=None) == -1 and b'null' in lib.dlwpcs_last_error()
    assert call(d, tab=TAB + 8) == -1 and b'Legendre table is not aligned' in lib.dlwpcs_last_error()
    assert call(d, tw=TW + 4) == -1 and b'twiddle table is not aligned' in lib.dlwpcs_last_error()
    assert call(d, a=None) == -1 and call(d, out=None) == -1
    assert call(d, a=A + 2) == -1 and b'4-byte' in lib.dlwpcs_last_error()
    assert call(d, scr=None) == -1 and call(d, scr=SCR + 8) == -1 and b'scratch' in lib.dlwpcs_last_error()
    d.n_dims = nat.SCORE_MAX_DIMS + 1
    assert call(d) == -1 and b'n_dims' in lib.dlwpcs_last_error()
    empty = _desc(fields=3)
    empty.ext[0] = 0
    assert call(empty) == 0                                             # no field: nothing to do, no launch
