"""
Winds, vorticity / divergence and gradients on the host (DLWP.verify.spherical_uv / spherical_vrtdiv / spherical_gradient with numpy
and labelled inputs) against facts the host twin did not produce, their refusals, and the host-side validation of
dlwpcs_sht_vector_synthesis / dlwpcs_sht_vector_analysis / dlwpcs_barotropic_flux / dlwpcs_barotropic_update through ctypes
(argument errors are caught before any launch: no device is needed).
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
A_EARTH = 6371200.


@pytest.mark.parametrize('kind,nlat,L', [('gauss', 16, 32), ('clenshaw-curtis', 17, 36), ('fejer', 18, 36)])
def test_solid_body_rotation(kind, nlat, L):
    """zeta = 2 w mu is the rotation u = a w cos(phi), v = 0"""
    lat = R.latitudes(kind, nlat)
    w = 7.848e-6
    zeta = np.repeat(2 * w * R.sin_lat(kind, nlat)[:, None], L, axis=1)
    u, v = verify.spherical_uv(verify.spherical_analysis(zeta, lat=lat), None, lat, L)
    assert np.abs(u - A_EARTH * w * np.cos(np.radians(lat))[:, None]).max() <= 1e-12 * A_EARTH * w
    assert np.abs(v).max() <= 1e-12 * A_EARTH * w


def test_gradient_has_no_curl_and_its_divergence_is_the_laplacian():
    rng = np.random.default_rng(3)
    c = S.random_packed(rng, T - 1, (4,), slope=1.0)                            # degrees <= T - 1: the gradient stays within T
    keep = [spharm.packed_row(m, n, T) for m in range(T) for n in range(m, T)]
    full = np.zeros((4, ROWS), dtype=complex)
    full[:, keep] = c
    x = verify.spherical_synthesis(full, LAT, L)
    gx, gy = verify.spherical_gradient(x, lat=LAT)
    assert gx.shape == x.shape and gy.shape == x.shape
    vrt, div = verify.spherical_vrtdiv(gx, gy, lat=LAT)
    lap = verify.spherical_analysis(verify.spherical_laplacian(x, lat=LAT), lat=LAT)
    scale = np.abs(lap).max()
    assert np.abs(vrt).max() <= 1e-12 * scale
    assert np.abs(div - lap).max() <= 1e-12 * scale
    # the zonal derivative of cos(phi) cos(lambda) / radius, exactly
    lon = 2 * np.pi * np.arange(L) / L
    y = np.cos(np.radians(LAT))[:, None] * np.cos(lon)[None, :]
    gx, gy = verify.spherical_gradient(y, lat=LAT, radius=2.0)
    assert np.abs(gx - (-np.sin(lon)[None, :] * np.ones((NLAT, 1))) / 2.0).max() <= 1e-13
    assert np.abs(gy - (-np.sin(np.radians(LAT))[:, None] * np.cos(lon)[None, :]) / 2.0).max() <= 1e-13
    # grid axes anywhere, latitudes in either direction
    xt = np.ascontiguousarray(np.moveaxis(x, 0, -1)[::-1])
    g2 = verify.spherical_gradient(xt, lat=LAT[::-1], lat_axis=0, lon_axis=1)
    g1 = verify.spherical_gradient(x, lat=LAT)
    for a, b in zip(g1, g2):
        assert b.shape == xt.shape and np.abs(np.moveaxis(b[::-1], -1, 0) - a).max() <= 1e-12 * np.abs(a).max()


def test_holes_and_absent_operands():
    rng = np.random.default_rng(4)
    u, v = rng.standard_normal((2, 3, NLAT, L))
    vrt, div = verify.spherical_vrtdiv(u, v, lat=LAT)
    assert vrt.shape == (3, ROWS) and vrt.dtype == np.complex128
    uh = u.copy()
    uh[1, 2, 3] = np.nan
    vh, dh = verify.spherical_vrtdiv(uh, v, lat=LAT)
    assert np.isnan(vh[1]).all() and np.isnan(dh[1]).all()
    assert np.array_equal(vh[[0, 2]], vrt[[0, 2]]) and np.array_equal(dh[[0, 2]], div[[0, 2]])
    u1, v1 = verify.spherical_uv(vrt, None, LAT, L)
    u2, v2 = verify.spherical_uv(None, div, LAT, L)
    u3, v3 = verify.spherical_uv(vrt, div, LAT, L)
    assert np.abs(u1 + u2 - u3).max() <= 1e-9 * np.abs(u3).max() and np.abs(v1 + v2 - v3).max() <= 1e-9 * np.abs(v3).max()


def test_labelled_inputs_keep_their_labels():
    rng = np.random.default_rng(5)
    lon = np.arange(L) * 360.0 / L
    coords = {'time': np.arange(3), 'lat': LAT, 'lon': lon}
    u = Forecast(rng.standard_normal((3, L, NLAT)), ('time', 'lon', 'lat'), coords, name='u')
    v = Forecast(rng.standard_normal((3, L, NLAT)), ('time', 'lon', 'lat'), coords, name='v')
    vrt, div = verify.spherical_vrtdiv(u, v)
    assert vrt.dims == ('time', 'coefficient') and div.dims == vrt.dims and np.array_equal(vrt.coords['time'], np.arange(3))
    ref = verify.spherical_vrtdiv(np.moveaxis(u.values, 1, 2), np.moveaxis(v.values, 1, 2), lat=LAT)
    assert np.array_equal(vrt.values, ref[0]) and np.array_equal(div.values, ref[1])
    uu, vv = verify.spherical_uv(vrt, div, LAT, L)
    assert uu.dims == ('time', 'lat', 'lon') and vv.dims == uu.dims
    assert np.array_equal(uu.coords['lat'], LAT) and np.allclose(uu.coords['lon'], lon) and np.array_equal(uu.coords['time'], np.arange(3))
    gx, gy = verify.spherical_gradient(u)
    assert gx.dims == u.dims and gy.dims == u.dims and np.array_equal(gx.coords['lat'], LAT)
    assert np.array_equal(gx.values, np.moveaxis(verify.spherical_gradient(np.moveaxis(u.values, 1, 2), lat=LAT)[0], 1, 2))


def test_refusals():
    x = np.zeros((3, NLAT, L))
    with pytest.raises(ValueError, match='neither'):
        verify.spherical_vrtdiv(x, x, lat=np.linspace(-80., 80., NLAT))
    with pytest.raises(ValueError, match='neither'):
        spharm.derivative_table(np.linspace(-80., 80., NLAT), 3)
    with pytest.raises(ValueError, match='latitudes'):
        verify.spherical_gradient(x)
    with pytest.raises(ValueError, match='one shape'):
        verify.spherical_vrtdiv(x, x[:2], lat=LAT)
    with pytest.raises(ValueError, match='above'):
        verify.spherical_vrtdiv(x, x, lat=LAT, truncation=T + 1)
    with pytest.raises(ValueError, match='both absent'):
        verify.spherical_uv(None, None, LAT, L)
    with pytest.raises(ValueError, match='truncation'):
        verify.spherical_uv(np.zeros((2, ROWS + 1), dtype=complex), None, LAT, L)
    with pytest.raises(ValueError, match='one shape'):
        verify.spherical_uv(np.zeros((2, ROWS), dtype=complex), np.zeros((3, ROWS), dtype=complex), LAT, L)
    with pytest.raises(ValueError, match='truncation'):
        spharm.zonal_table(LAT, T + 1)
    tr = spharm.SphericalTransform(LAT, L)
    with pytest.raises(ValueError, match='potential'):
        tr.vector_synthesis(None, None)
    with pytest.raises(ValueError, match='want'):
        tr.vector_analysis(x, x, want=('curl',))
    with pytest.raises(ValueError, match='response'):
        tr.vector_analysis(x, x, response=np.ones(T))


def test_ops_argument_checks():
    import torch
    from DLWP import _native as nat, ops
    tr = spharm.SphericalTransform(LAT, L)
    c = torch.zeros((3, ROWS), dtype=torch.complex64)
    g = torch.zeros((3, NLAT, L))
    with pytest.raises(nat.NativeError):                                        # host tensors: there is no fall-back
        ops.spherical_vector_synthesis(c, None, tr)
    with pytest.raises(nat.NativeError):
        ops.spherical_vector_analysis(g, g, tr)
    with pytest.raises(nat.NativeError):
        ops.barotropic_flux(g, g, g, torch.zeros(NLAT))
    with pytest.raises(nat.NativeError):
        ops.barotropic_update(c, c.clone(), c.clone(), torch.zeros(ROWS), 600., 0.04, True)
    with pytest.raises(ValueError, match='both potentials'):
        ops.spherical_vector_synthesis(None, None, tr)
    with pytest.raises(TypeError, match='complex64'):
        ops.spherical_vector_synthesis(c.to(torch.complex128), None, tr)
    with pytest.raises(ValueError, match='coefficients'):
        ops.spherical_vector_synthesis(c[:, :-1], None, tr)
    with pytest.raises(TypeError, match='SphericalTransform'):
        ops.spherical_vector_synthesis(c, None, None)
    with pytest.raises(ValueError, match='want'):
        ops.spherical_vector_analysis(g, g, tr, want=())
    with pytest.raises(ValueError, match='want'):
        ops.spherical_vector_analysis(g, g, tr, want=('vrt', 'vrt'))
    with pytest.raises(TypeError, match='float32'):
        ops.barotropic_flux(g.double(), g, g, torch.zeros(NLAT))
    with pytest.raises(TypeError, match='complex64'):
        ops.barotropic_update(g, g, g, torch.zeros(ROWS), 600., 0.04, True)


def test_overlap_of_two_views():
    """what the wrappers refuse outputs by: apart, provably interleaved, or possibly overlapping"""
    import torch
    from DLWP import ops
    base = torch.zeros((4, 2, 6, 8))
    assert ops._may_overlap(base, base) and ops._may_overlap(base[1:], base[:2]) and ops._may_overlap(base[:, 0], base)
    assert not ops._may_overlap(base[:2], base[2:])                              # address ranges apart
    assert not ops._may_overlap(base[:, 0], base[:, 1])                          # two slices of one interleaved buffer
    assert not ops._may_overlap(base[:, 0, :, :4], base[:, 0, :, 4:])            # interleaved along longitude
    assert not ops._may_overlap(base[:, 1, 2:], base[:, 1, :2])
    assert ops._may_overlap(base[:, 0, :, :5], base[:, 0, :, 4:])                # one shared column
    assert ops._may_overlap(base[:, :, 0], base[:, 0])
    assert not ops._may_overlap(base[:0], base)                                  # nothing to write
    flat = torch.zeros(64)
    assert ops._may_overlap(flat[::2], flat[::4]) and not ops._may_overlap(flat[::2], flat[1::2])
    # a view with a negative stride is never shown to be apart (torch makes none today -- flip() copies -- so a stand-in with
    # the four members the check reads)
    class Reversed(object):
        shape, numel = (3,), staticmethod(lambda: 3)
        stride, data_ptr = staticmethod(lambda: (-1,)), staticmethod(lambda: flat.data_ptr() + 4 * 40)
    assert ops._may_overlap(Reversed(), flat[:3]) and ops._may_overlap(flat[:3], Reversed())


def _desc(nlat=NLAT, n_lon=L, trunc=T, fields=3):
    from DLWP import ops
    dims = ops.spectrum_dims((fields,), [(nlat * n_lon,), (nlat * n_lon,)], ())
    return ops.sht_desc(nlat, n_lon, trunc, dims, (n_lon, n_lon))


def test_argument_validation_on_the_host():
    """every argument error of the four entry points comes back before a launch with a message: fake (never dereferenced)
    device addresses suffice"""
    from DLWP import _native as nat
    lib = nat.lib()
    nlp = (NLAT + 3) // 4 * 4
    A, B, TW, TD, TQ, SCR, U, V, RESP = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000, 0x90000

    d = _desc()
    assert lib.dlwpcs_sht_vector_synthesis_scratch_bytes(ctypes.byref(d)) == 2 * 3 * (T + 1) * 2 * nlp * 4
    assert lib.dlwpcs_sht_vector_analysis_scratch_bytes(ctypes.byref(d)) == 2 * 3 * (T + 1) * 2 * nlp * 4 + 3 * NLAT * 4

    def syn(desc, a=A, b=B, rp=RESP, rc=RESP, tw=TW, td=TD, tq=TQ, scr=SCR, u=U, v=V):
        return lib.dlwpcs_sht_vector_synthesis(ctypes.byref(desc), a, b, rp, rc, tw, td, tq, scr, u, v, None)

    def ana(desc, u=U, v=V, r=RESP, tw=TW, td=TD, tq=TQ, scr=SCR, z=A, dv=B, skipped=None):
        return lib.dlwpcs_sht_vector_analysis(ctypes.byref(desc), u, v, r, tw, td, tq, scr, z, dv, skipped, None)

    for call, query in ((syn, lib.dlwpcs_sht_vector_synthesis_scratch_bytes), (ana, lib.dlwpcs_sht_vector_analysis_scratch_bytes)):
        for bad, word in ((_desc(trunc=18), b'truncation'), (_desc(trunc=-1), b'truncation'), (_desc(n_lon=1, trunc=0), b'longitudes'),
                          (_desc(nlat=1, trunc=0), b'latitudes')):
            assert call(bad) == -1 and word in lib.dlwpcs_last_error()
            assert query(ctypes.byref(bad)) == 0
        for bad in (_desc(n_lon=1730), _desc(nlat=nat.SHT_MAX_NLAT + 1)):
            assert call(bad) == -2 and b'serves' in lib.dlwpcs_last_error()
        assert call(d, tw=None) == -1 and b'null' in lib.dlwpcs_last_error()
        assert call(d, td=None) == -1 and b'null' in lib.dlwpcs_last_error()
        assert call(d, tq=None) == -1 and b'null' in lib.dlwpcs_last_error()
        assert call(d, tw=TW + 4) == -1 and b'8 bytes' in lib.dlwpcs_last_error()
        assert call(d, td=TD + 4) == -1 and b'16 bytes' in lib.dlwpcs_last_error()
        assert call(d, tq=TQ + 8) == -1 and b'16 bytes' in lib.dlwpcs_last_error()
        assert call(d, scr=None) == -1 and b'scratch' in lib.dlwpcs_last_error()
        assert call(d, scr=SCR + 8) == -1 and b'scratch' in lib.dlwpcs_last_error()
        assert call(d, u=None) == -1 and b'null' in lib.dlwpcs_last_error()
        assert call(d, v=None) == -1 and b'null' in lib.dlwpcs_last_error()
        assert call(d, u=U + 2) == -1 and b'4-byte' in lib.dlwpcs_last_error()
        assert call(_desc(fields=0), u=None, v=None, scr=None) == 0             # zero fields: success without a launch
    assert syn(d, a=None, b=None) == -1 and b'both potentials' in lib.dlwpcs_last_error()
    assert syn(d, a=A + 4) == -1 and b'8-byte' in lib.dlwpcs_last_error()
    assert syn(d, rp=RESP + 1) == -1 and b'4-byte' in lib.dlwpcs_last_error()
    assert ana(d, z=None, dv=None) == -1 and b'both outputs' in lib.dlwpcs_last_error()
    assert ana(d, dv=B + 4) == -1 and b'8-byte' in lib.dlwpcs_last_error()
    assert ana(d, skipped=0x1002) == -1 and b'4-byte' in lib.dlwpcs_last_error()

    def flux(fields=3, nlat=NLAT, n_lon=L, f=A, z=B, u=U, v=V, F=TD, G=TQ):
        return lib.dlwpcs_barotropic_flux(fields, nlat, n_lon, f, z, u, v, F, G, None)

    assert flux(fields=-1) == -1 and b'fields' in lib.dlwpcs_last_error()
    assert flux(nlat=0) == -1 and flux(n_lon=0) == -1
    assert flux(fields=1 << 31) == -2 and b'too many' in lib.dlwpcs_last_error()
    assert flux(f=None) == -1 and b'null' in lib.dlwpcs_last_error()
    assert flux(G=None) == -1 and b'null' in lib.dlwpcs_last_error()
    assert flux(u=U + 1) == -1 and b'4-byte' in lib.dlwpcs_last_error()
    assert flux(fields=1 << 20, nlat=1000, n_lon=(1 << 31) - 1) == -2 and b'workgroups' in lib.dlwpcs_last_error()
    assert flux(fields=0, z=None) == 0

    def upd(fields=3, rows=ROWS, damp=A, dt=600., rc=0.04, first=1, tend=B, z=U, zp=V):
        return lib.dlwpcs_barotropic_update(fields, rows, damp, dt, rc, first, tend, z, zp, None)

    assert upd(fields=-1) == -1 and upd(rows=0) == -1
    assert upd(rows=1 << 31) == -2 and b'too many' in lib.dlwpcs_last_error()
    assert upd(dt=float('nan')) == -1 and b'NaN' in lib.dlwpcs_last_error()
    assert upd(damp=None) == -1 and b'null' in lib.dlwpcs_last_error()
    assert upd(zp=None) == -1 and b'null' in lib.dlwpcs_last_error()
    assert upd(zp=U) == -1 and b'one buffer' in lib.dlwpcs_last_error()
    assert upd(tend=U) == -1 and b'one buffer' in lib.dlwpcs_last_error()
    assert upd(tend=V) == -1 and b'one buffer' in lib.dlwpcs_last_error()
    assert upd(fields=(1 << 31) - 1, rows=(1 << 31) - 1) == -2 and b'workgroups' in lib.dlwpcs_last_error()
    assert upd(tend=B + 4) == -1 and b'8-byte' in lib.dlwpcs_last_error()
    assert upd(damp=A + 2) == -1 and b'4-byte' in lib.dlwpcs_last_error()
    assert upd(fields=0, tend=None) == 0
