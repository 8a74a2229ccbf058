"""
Spherical-harmonic analysis, synthesis, filter and Laplacian on the host (DLWP.verify with numpy and labelled inputs) against the
float64 reference of sht_synth_ref.py, their refusals, and the host-side validation of dlwpcs_sht_analysis / dlwpcs_sht_synthesis
through ctypes (descriptor errors are caught before any launch: no device is needed).
"""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sht_ref as R             # noqa: E402
import sht_synth_ref as S       # noqa: E402

from DLWP import verify      # noqa: E402
from DLWP.model.extensions import Forecast     # noqa: E402
from DLWP.remap import spharm   # noqa: E402

KIND, NLAT, L, T = 'clenshaw-curtis', 17, 36, 8
LAT = R.latitudes(KIND, NLAT)
ROWS = S.packed_rows(T)


def test_analysis_and_synthesis_on_numpy_inputs():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((3, 4, NLAT, L)) + 2.0
    c = verify.spherical_analysis(x, lat=LAT)
    assert c.shape == (3, 4, ROWS) and c.dtype == np.complex128
    assert np.abs(c - S.analysis(x, KIND, T)).max() <= 1e-13
    low = verify.spherical_analysis(x, lat=LAT, truncation=5)
    keep = [spharm.packed_row(m, n, T) for m in range(6) for n in range(m, 6)]
    assert np.abs(low - c[..., keep]).max() <= 1e-14                       # a smaller truncation is a subset of the larger
    y = verify.spherical_synthesis(c, LAT, L)
    assert y.shape == x.shape and y.dtype == np.float64
    assert np.abs(y - S.synthesis(c, KIND, NLAT, L)).max() <= 1e-12
    assert np.abs(verify.spherical_analysis(y, lat=LAT) - c).max() <= 1e-12
    resp = rng.standard_normal(T + 1)
    assert np.abs(verify.spherical_synthesis(c, LAT, L, response=resp) - S.synthesis(c, KIND, NLAT, L, resp)).max() <= 1e-12
    # grid axes anywhere, latitudes in either direction
    xt = np.ascontiguousarray(x.transpose(2, 0, 3, 1)[::-1])
    assert np.abs(verify.spherical_analysis(xt, lat=LAT[::-1], lat_axis=0, lon_axis=2) - c).max() <= 1e-13
    assert np.abs(verify.spherical_synthesis(c, LAT[::-1], L) - y[..., ::-1, :]).max() <= 1e-12
    # a field with a hole: NaN coefficients, a flag, a NaN field back; the others untouched
    xh = x.copy()
    xh[1, 2, 3, 4] = np.nan
    xh[2, 0, 0, 0] = np.inf
    ch, flags = verify.spherical_analysis(xh, lat=LAT, return_count=True)
    assert flags.dtype == np.int32 and flags.sum() == 2 and flags[1, 2] == 1 and flags[2, 0] == 1
    assert np.isnan(ch[1, 2]).all() and np.isnan(ch[2, 0]).all()
    ok = flags == 0
    assert np.array_equal(ch[ok], c[ok])
    back = verify.spherical_filter(xh, lat=LAT)
    assert np.isnan(back[1, 2]).all() and np.isnan(back[2, 0]).all() and not np.isnan(back[ok]).any()


def test_filter_and_laplacian():
    rng = np.random.default_rng(2)
    c = S.random_packed(rng, T, (2, 3))
    x = S.synthesis(c, KIND, NLAT, L)                                      # band-limited to T
    assert np.abs(verify.spherical_filter(x, lat=LAT) - x).max() <= 1e-11
    cut = verify.spherical_filter(x, lat=LAT, cutoff=4)
    low = verify.spherical_analysis(x, lat=LAT, truncation=4)              # the analysis at the lower truncation
    assert cut.shape == x.shape and np.abs(cut - verify.spherical_synthesis(low, LAT, L)).max() <= 1e-11
    assert np.abs(verify.spherical_filter(x, lat=LAT, truncation=4) - cut).max() <= 1e-11
    assert np.abs(verify.spherical_filter(x, lat=LAT, cutoff=T + 3) - x).max() <= 1e-11
    resp = np.linspace(1.0, 0.0, T + 1)
    assert np.abs(verify.spherical_filter(x, lat=LAT, response=resp) - S.synthesis(c, KIND, NLAT, L, resp)).max() <= 1e-11
    # axes anywhere and flipped latitudes: the output has the input's shape and axis order
    xt = np.ascontiguousarray(x.transpose(3, 0, 2, 1)[:, :, ::-1])         # (lon, 2, lat south first, 3)
    got = verify.spherical_filter(xt, lat=LAT[::-1], lat_axis=2, lon_axis=0, cutoff=4)
    assert got.shape == xt.shape and np.abs(got - cut.transpose(3, 0, 2, 1)[:, :, ::-1]).max() <= 1e-11
    # the Laplacian: -n (n + 1) / a^2 per degree; its inverse undoes it apart from the mean
    a = 6371200.
    lap = verify.spherical_laplacian(x, lat=LAT)
    n = np.arange(T + 1)
    assert np.abs(lap - S.synthesis(c, KIND, NLAT, L, -n * (n + 1) / a ** 2)).max() <= 1e-11 / a ** 2 * T * (T + 1)
    back = verify.spherical_laplacian(lap, lat=LAT, inverse=True)
    mean = c[..., 0].real[..., None, None]
    assert np.abs(back - (x - mean)).max() <= 1e-9
    assert np.abs(verify.spherical_laplacian(x, lat=LAT, radius=1.0) - a ** 2 * lap).max() <= 1e-9


def test_labelled_inputs_keep_their_labels():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((3, L, NLAT, 2))
    coords = {'f_hour': np.array([6, 12, 18]), 'lon': np.arange(L) * 10., 'lat': LAT, 'varlev': np.array(['z', 't'])}
    fx = Forecast(x, ('f_hour', 'lon', 'lat', 'varlev'), coords)
    c = verify.spherical_analysis(fx)
    assert c.dims == ('f_hour', 'varlev', 'coefficient') and c.values.shape == (3, 2, ROWS)
    assert np.array_equal(c.values, verify.spherical_analysis(x, lat=LAT, lat_axis=2, lon_axis=1))
    y = verify.spherical_synthesis(c, LAT, L)
    assert y.dims == ('f_hour', 'varlev', 'lat', 'lon') and np.array_equal(y.coords['lat'], LAT)
    assert np.array_equal(y.coords['varlev'], coords['varlev']) and np.allclose(y.coords['lon'], coords['lon'])
    f = verify.spherical_filter(fx, cutoff=3)
    assert f.dims == fx.dims and f.values.shape == x.shape and all(np.array_equal(f.coords[k], coords[k]) for k in coords)
    assert np.array_equal(f.values, verify.spherical_filter(x, lat=LAT, lat_axis=2, lon_axis=1, cutoff=3))
    assert np.abs(np.moveaxis(f.values, (2, 1), (-2, -1)) - verify.spherical_synthesis(c, LAT, L, spharm.truncation_response(T, 3)).values
                  ).max() <= 1e-12
    assert verify.spherical_laplacian(fx).dims == fx.dims


def test_refusals():
    x = np.zeros((3, NLAT, L))
    with pytest.raises(ValueError, match='mutually exclusive'):
        verify.spherical_filter(x, lat=LAT, cutoff=3, response=np.ones(T + 1))
    with pytest.raises(ValueError, match='negative'):
        verify.spherical_filter(x, lat=LAT, cutoff=-1)
    with pytest.raises(ValueError, match='response'):
        verify.spherical_filter(x, lat=LAT, response=np.ones(T))
    with pytest.raises(ValueError, match='above'):
        verify.spherical_filter(x, lat=LAT, truncation=T + 1)
    with pytest.raises(ValueError, match='latitudes'):
        verify.spherical_analysis(x)
    with pytest.raises(ValueError, match='neither'):
        verify.spherical_analysis(x, lat=np.linspace(-80., 80., NLAT))
    with pytest.raises(ValueError, match='truncation'):
        verify.spherical_synthesis(np.zeros((2, ROWS + 1), dtype=complex), LAT, L)
    with pytest.raises(ValueError, match='response'):
        verify.spherical_synthesis(np.zeros((2, ROWS), dtype=complex), LAT, L, response=np.ones(3))
    with pytest.raises(ValueError, match='longitudes'):
        verify.spherical_synthesis(np.zeros((2, ROWS), dtype=complex), LAT, 16)


def test_device_functions_refuse_host_tensors():
    import torch
    from DLWP import _native as nat, ops
    tr = spharm.SphericalTransform(LAT, L)
    with pytest.raises(nat.NativeError):
        ops.spherical_analysis(torch.zeros((3, NLAT, L)), tr)
    with pytest.raises(nat.NativeError):
        ops.spherical_synthesis(torch.zeros((3, ROWS), dtype=torch.complex64), tr)


def _desc(nlat=NLAT, n_lon=L, trunc=T, fields=3):
    from DLWP import ops
    dims = ops.spectrum_dims((fields,), [(nlat * n_lon,), (0,)], ())
    return ops.sht_desc(nlat, n_lon, trunc, dims, (n_lon, 0))


def _sdesc(nlat=NLAT, n_lon=L, trunc=T, fields=3):
    from DLWP import ops
    return ops.sht_synthesis_desc(nlat, n_lon, trunc, ops.spectrum_dims((fields,), [(nlat * n_lon,)], ()), n_lon)


def test_descriptor_validation_on_the_host():
    """every descriptor error of the two entry points comes back before a launch with a message: fake (never dereferenced)
    device addresses suffice"""
    from DLWP import _native as nat
    lib = nat.lib()
    nlp = (NLAT + 3) // 4 * 4
    A, TW, TAB, OUT, SCR, COEF, RESP = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000

    d = _desc()
    assert lib.dlwpcs_sht_analysis_scratch_bytes(ctypes.byref(d)) == 3 * (T + 1) * 2 * nlp * 4 + 3 * NLAT * 4

    def ana(desc, a=A, tw=TW, tab=TAB, scr=SCR, coef=COEF, skipped=None):
        return lib.dlwpcs_sht_analysis(ctypes.byref(desc), a, tw, tab, scr, coef, skipped, None)

    s = _sdesc()
    assert (s.nlat, s.L, s.T, s.n_dims, s.ext[0], s.stride[0], s.lat_stride) == (NLAT, L, T, 1, 3, NLAT * L, L)
    assert lib.dlwpcs_sht_synthesis_scratch_bytes(ctypes.byref(s)) == 3 * (T + 1) * 2 * nlp * 4

    def syn(desc, coef=COEF, resp=RESP, tw=TW, tab=TAB, scr=SCR, out=OUT):
        return lib.dlwpcs_sht_synthesis(ctypes.byref(desc), coef, resp, tw, tab, scr, out, None)

    for call, make, query in ((ana, _desc, lib.dlwpcs_sht_analysis_scratch_bytes), (syn, _sdesc, lib.dlwpcs_sht_synthesis_scratch_bytes)):
        for bad, word in ((make(trunc=18), b'truncation'), (make(trunc=-1), b'truncation'), (make(n_lon=1, trunc=0), b'longitudes'),
                          (make(nlat=1, trunc=0), b'latitudes')):
            assert call(bad) == -1 and word in lib.dlwpcs_last_error()
            assert query(ctypes.byref(bad)) == 0
        for bad in (make(n_lon=1730), make(nlat=nat.SHT_MAX_NLAT + 1)):
            assert call(bad) == -2 and b'serves' in lib.dlwpcs_last_error()
        good = make()
        assert call(good, tab=None) == -1 and b'null' in lib.dlwpcs_last_error()
        assert call(good, tw=None) == -1 and b'null' in lib.dlwpcs_last_error()
        assert call(good, tab=TAB + 8) == -1 and b'Legendre table is not aligned' in lib.dlwpcs_last_error()
        assert call(good, tw=TW + 4) == -1 and b'twiddle table is not aligned' in lib.dlwpcs_last_error()
        assert call(good, coef=None) == -1 and b'null' in lib.dlwpcs_last_error()
        assert call(good, coef=COEF + 4) == -1 and b'8-byte' in lib.dlwpcs_last_error()
        assert call(good, scr=None) == -1 and call(good, scr=SCR + 8) == -1 and b'scratch' in lib.dlwpcs_last_error()
        over = make()
        over.n_dims = nat.SCORE_MAX_DIMS + 1
        assert call(over) == -1 and b'n_dims' in lib.dlwpcs_last_error()
        empty = make()
        empty.ext[0] = 0
        assert call(empty) == 0                                            # no field: nothing to do, no launch
    assert ana(d, a=None) == -1 and ana(d, a=A + 2) == -1 and b'4-byte' in lib.dlwpcs_last_error()
    assert syn(s, out=None) == -1 and syn(s, out=OUT + 2) == -1 and b'4-byte' in lib.dlwpcs_last_error()
    assert syn(s, resp=RESP + 1) == -1 and b'4-byte' in lib.dlwpcs_last_error()
    assert syn(_sdesc(trunc=18)) == -1 and b'sht_synthesis' in lib.dlwpcs_last_error()
    assert ana(_desc(trunc=18)) == -1 and b'sht_analysis' in lib.dlwpcs_last_error()
