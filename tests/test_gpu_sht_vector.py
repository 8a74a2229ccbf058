"""
dlwpcs_sht_vector_synthesis and dlwpcs_sht_vector_analysis on the device against the float64 host twin
(DLWP.remap.spharm.SphericalTransform.vector_synthesis / vector_analysis) within the bounds derived in sht_vector_ref.py, and the
two streaming kernels of the barotropic model bit for bit against their float32 restatement.  Every comparison prints the largest
fraction of the bound it saw.  Shapes: sht_vector_ref.GPU_CASES.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sht_ref as R          # noqa: E402
import sht_synth_ref as S    # noqa: E402
import sht_vector_ref as V   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_TRANSFORMS = {}
TINY = np.finfo(np.float64).tiny


def _transform(kind, nlat, L, T=None, south_first=False):
    from DLWP.remap import spharm
    key = (kind, nlat, L, T, south_first)
    if key not in _TRANSFORMS:
        _TRANSFORMS[key] = spharm.SphericalTransform(R.latitudes(kind, nlat, south_first), L, T)
    return _TRANSFORMS[key]


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bits(t):
    t = t.detach()
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.contiguous().view(torch.int32).cpu().numpy()


def _same_bits(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def _check_synthesis(got, a, b, rp, rc, tr, kind, south, what):
    """device (u, v) against the host twin within synthesis_bound; returns the largest fraction"""
    f64 = lambda x: None if x is None else x.astype(np.float64)          # noqa: E731
    c128 = lambda x: None if x is None else x.astype(np.complex128)      # noqa: E731
    ref = tr.vector_synthesis(c128(a), c128(b), f64(rp), f64(rc))
    lim = V.synthesis_bound(a, b, f64(rp), f64(rc), kind, tr.nlat, tr.truncation)
    worst = 0.0
    for g, r, l in zip(got, ref, lim):
        l = (l[..., ::-1] if south else l)[..., None]
        err = np.abs(g.cpu().numpy().astype(np.float64) - r)
        frac = float((err / np.maximum(l, TINY)).max())
        assert (err <= l).all(), '%s: synthesis at %.3g of the bound' % (what, frac)
        worst = max(worst, frac)
    print('%s: synthesis, largest |error| / bound = %.4f' % (what, worst))
    return worst


def _check_analysis(got, u, v, resp, tr, kind, south, what, want=('vrt', 'div')):
    """device coefficients against the host twin within analysis_bound (Re and Im each); returns the largest fraction"""
    u64, v64 = u.astype(np.float64), v.astype(np.float64)
    r64 = None if resp is None else resp.astype(np.float64)
    ref = dict(zip(('vrt', 'div'), tr.vector_analysis(u64, v64, r64)))
    flip = (lambda x: x[..., ::-1, :]) if south else (lambda x: x)
    lim = dict(zip(('vrt', 'div'), V.analysis_bound(flip(u64), flip(v64), r64, kind, tr.truncation)))
    worst = 0.0
    for name, g in zip(want, got):
        g = g.cpu().numpy()
        err = np.maximum(np.abs(g.real.astype(np.float64) - ref[name].real), np.abs(g.imag.astype(np.float64) - ref[name].imag))
        frac = float((err / np.maximum(lim[name], TINY)).max())
        assert (err <= lim[name]).all(), '%s: %s at %.3g of the bound' % (what, name, frac)
        worst = max(worst, frac)
    print('%s: analysis, largest |error| / bound = %.4f' % (what, worst))
    return worst


@pytest.mark.parametrize('L', [12, 37, 72, 100, 264])
def test_shape_grid(L):
    from DLWP import ops
    cases = [(n, c) for n, c in enumerate(V.GPU_CASES) if c[2] == L]
    assert cases
    for n, (kind, nlat, L, T, fields, south) in cases:
        rng = np.random.default_rng(1000 * nlat + L + T)
        tr = _transform(kind, nlat, L, T, south)
        what = '%s %d x %d T=%d fields=%d south=%d' % (kind, nlat, L, T, fields, south)
        A = S.random_packed(rng, T, (fields,), slope=(n % 3) * 0.5).astype(np.complex64)
        B = S.random_packed(rng, T, (fields,), slope=(n % 2) * 0.5).astype(np.complex64)
        rp = rng.standard_normal(T + 1).astype(np.float32) if n % 2 else None
        rc = rng.standard_normal(T + 1).astype(np.float32) if n % 3 else None
        both = ops.spherical_vector_synthesis(_dev(A), _dev(B), tr, _dev(rp), _dev(rc))
        _check_synthesis(both, A, B, rp, rc, tr, kind, south, what)
        if n % 2:                                                        # either potential absent
            _check_synthesis(ops.spherical_vector_synthesis(_dev(A), None, tr, _dev(rp)), A, None, rp, None, tr, kind, south, what + ' psi')
        else:
            _check_synthesis(ops.spherical_vector_synthesis(None, _dev(B), tr, None, _dev(rc)), None, B, None, rc, tr, kind, south, what + ' chi')
        u = R.make_field(rng, (fields, nlat, L), 'red' if n % 2 else 'white', 20.0 if n % 3 == 0 else 0.0)
        v = R.make_field(rng, (fields, nlat, L), 'white', 0.0)
        z, d, flags = ops.spherical_vector_analysis(_dev(u), _dev(v), tr, _dev(rp), counts=True)
        assert not bool(flags.any())
        _check_analysis((z, d), u, v, rp, tr, kind, south, what)
        # either output absent: the other keeps its bits (its accumulators see the same instructions in the same order)
        assert _same_bits(ops.spherical_vector_analysis(_dev(u), _dev(v), tr, _dev(rp), want=('vrt',))[0], z)
        assert _same_bits(ops.spherical_vector_analysis(_dev(u), _dev(v), tr, _dev(rp), want=('div',))[0], d)


@pytest.mark.parametrize('fields', [1, 32, 33, 65])
def test_repeatable_null_response_and_independent_of_the_other_fields(fields):
    from DLWP import ops
    rng = np.random.default_rng(fields)
    tr = _transform('clenshaw-curtis', 33, 72)
    T = tr.truncation
    u, v = _dev(R.make_field(rng, (fields, 33, 72), 'red')), _dev(R.make_field(rng, (fields, 33, 72)))
    a = _dev(S.random_packed(rng, T, (fields,)).astype(np.complex64))
    b = _dev(S.random_packed(rng, T, (fields,)).astype(np.complex64))
    a1, a2 = ops.spherical_vector_analysis(u, v, tr), ops.spherical_vector_analysis(u, v, tr)
    s1, s2 = ops.spherical_vector_synthesis(a, b, tr), ops.spherical_vector_synthesis(a, b, tr)
    assert all(_same_bits(x, y) for x, y in zip(a1 + s1, a2 + s2)), 'two runs of one call differ'
    ones = torch.ones(T + 1, dtype=torch.float32, device=DEV)
    assert all(_same_bits(x, y) for x, y in zip(ops.spherical_vector_synthesis(a, b, tr, ones, ones), s1)), 'NULL is not ones'
    assert all(_same_bits(x, y) for x, y in zip(ops.spherical_vector_analysis(u, v, tr, ones), a1)), 'NULL is not ones'
    for others in (1, 33, 64):                                           # the last field among 1, 33 and 64 others
        mk = lambda x, new: torch.cat([new, x[-1:]])                    # noqa: E731
        uo, vo = (mk(x, _dev(R.make_field(rng, (others, 33, 72)))) for x in (u, v))
        ao, bo = (mk(x, _dev(S.random_packed(rng, T, (others,)).astype(np.complex64))) for x in (a, b))
        for x, y in zip(ops.spherical_vector_analysis(uo, vo, tr) + ops.spherical_vector_synthesis(ao, bo, tr), a1 + s1):
            assert _same_bits(x[-1], y[-1]), 'among %d others' % others


def test_element_paths_views_and_outs():
    from DLWP import ops
    rng = np.random.default_rng(7)
    for kind, nlat, L in (('fejer', 10, 12), ('clenshaw-curtis', 33, 72)):
        tr = _transform(kind, nlat, L)
        T = tr.truncation
        hu, hv = R.make_field(rng, (3, nlat, L)), R.make_field(rng, (3, nlat, L))
        a = _dev(S.random_packed(rng, T, (3,)).astype(np.complex64))
        # one element off a 16-byte line: the element loads and stores on the numbers the vector path has just served
        bufs = [torch.zeros(hu.size + 1, dtype=torch.float32, device=DEV) for _ in range(2)]
        xu, xv = (b[1:].view(3, nlat, L) for b in bufs)
        xu.copy_(torch.from_numpy(hu)); xv.copy_(torch.from_numpy(hv))
        assert xu.data_ptr() % 16 == 4
        want = ops.spherical_vector_analysis(_dev(hu), _dev(hv), tr)
        assert all(_same_bits(x, y) for x, y in zip(ops.spherical_vector_analysis(xu, xv, tr), want))
        assert all(_same_bits(x, y) for x, y in zip(ops.spherical_vector_analysis(xu, _dev(hv), tr), want))
        wu, wv = ops.spherical_vector_synthesis(a, None, tr)
        obuf = torch.full((hu.size + 1,), float('nan'), dtype=torch.float32, device=DEV)
        o = obuf[1:].view(3, nlat, L)
        ov = torch.empty((3, nlat, L), dtype=torch.float32, device=DEV)      # u by elements, v by 16-byte stores in one call
        ru, rv = ops.spherical_vector_synthesis(a, None, tr, out_u=o, out_v=ov)
        assert ru is o and rv is ov and _same_bits(o, wu) and _same_bits(ov, wv) and bool(torch.isnan(obuf[0]))
    kind, nlat, L = 'fejer', 10, 12
    tr = _transform(kind, nlat, L)
    T = tr.truncation
    # a latitude axis in the middle with longitude at unit stride (no copy), a strided leading axis, and a permuted view
    gu, gv = _dev(R.make_field(rng, (4, nlat, 6, L))), _dev(R.make_field(rng, (4, nlat, 6, L)))
    flat = ops.spherical_vector_analysis(gu.permute(0, 2, 1, 3).contiguous(), gv.permute(0, 2, 1, 3).contiguous(), tr)
    assert flat[0].shape == (4, 6, S.packed_rows(T)) and flat[0].dtype == torch.complex64
    assert all(_same_bits(x, y) for x, y in zip(ops.spherical_vector_analysis(gu, gv, tr, lat_axis=1), flat))
    part = ops.spherical_vector_analysis(gu[::2, :, 1::2], gv[::2, :, 1::2], tr, lat_axis=1)
    assert all(_same_bits(x, y[::2, 1::2]) for x, y in zip(part, flat))
    perm = ops.spherical_vector_analysis(gu.permute(3, 1, 0, 2), gv.permute(3, 1, 0, 2), tr, lat_axis=1, lon_axis=0)
    assert all(_same_bits(x, y) for x, y in zip(perm, flat))
    # outputs that are views with a latitude stride and permuted leading axes, each its own; what lies between is not written
    a, b = (_dev(S.random_packed(rng, T, (3, 5)).astype(np.complex64)) for _ in range(2))
    wu, wv = ops.spherical_vector_synthesis(a, b, tr)
    assert wu.shape == (3, 5, nlat, L) and wu.dtype == torch.float32
    store = torch.full((5, nlat, 3, 2, L + 4), float('nan'), dtype=torch.float32, device=DEV)
    view_u = store[:, :, :, 1, :L].permute(2, 0, 1, 3)
    store_v = torch.full((3, nlat, 5, L), float('nan'), dtype=torch.float32, device=DEV)
    view_v = store_v.permute(0, 2, 1, 3)
    ops.spherical_vector_synthesis(a, b, tr, out_u=view_u, out_v=view_v)
    assert _same_bits(view_u, wu) and _same_bits(view_v, wv)
    assert bool(torch.isnan(store[:, :, :, 0]).all()) and bool(torch.isnan(store[..., L:]).all())
    a7 = _dev(S.random_packed(rng, T, (7,)).astype(np.complex64))
    assert _same_bits(ops.spherical_vector_synthesis(a7[::6], None, tr)[0], ops.spherical_vector_synthesis(a7, None, tr)[0][::6])


def test_one_missing_field_among_33():
    from DLWP import ops
    rng = np.random.default_rng(23)
    kind, nlat, L = 'clenshaw-curtis', 19, 37
    tr = _transform(kind, nlat, L)
    for n, bits in enumerate(R.NAN_BITS[::2]):
        u, v = R.make_field(rng, (33, nlat, L)), R.make_field(rng, (33, nlat, L))
        holed = [u.copy(), v.copy()]
        bad = (5, 32, 17)[n]
        holed[n % 2].view(np.uint32)[bad, rng.integers(0, nlat), rng.integers(0, L)] = bits
        keep = [i for i in range(33) if i != bad]
        z, d, flags = ops.spherical_vector_analysis(_dev(holed[0]), _dev(holed[1]), tr, counts=True)
        cz, cd = ops.spherical_vector_analysis(_dev(u), _dev(v), tr)
        assert flags.cpu().numpy().tolist() == [int(i == bad) for i in range(33)]
        assert bool(torch.isnan(torch.view_as_real(z[bad])).all()) and bool(torch.isnan(torch.view_as_real(d[bad])).all())
        assert _same_bits(z[keep], cz[keep]) and _same_bits(d[keep], cd[keep])
        only, = ops.spherical_vector_analysis(_dev(holed[0]), _dev(holed[1]), tr, want=('div',))
        assert _same_bits(only, d)
        bu, bv = ops.spherical_vector_synthesis(z, d, tr)
        ku, kv = ops.spherical_vector_synthesis(cz, cd, tr)
        assert bool(torch.isnan(bu[bad]).all()) and bool(torch.isnan(bv[bad]).all())
        assert _same_bits(bu[keep], ku[keep]) and _same_bits(bv[keep], kv[keep])


def _chain_tolerances(links, propagated, scale):
    """the bound of a chain: the bounds of its last link, what the exact last link makes of the bound of the link before it, and
    1e-11 of the largest coefficient for the float64 identity itself (the round trip of the host twin holds to that: CPU test)"""
    return [a + p + 1e-11 * scale for a, p in zip(links, propagated)]


def _component_error(got, ref):
    return np.maximum(np.abs(got.real.astype(np.float64) - ref.real), np.abs(got.imag.astype(np.float64) - ref.imag))


def test_public_functions_agree_with_the_existing_calls():
    """spherical_uv, spherical_vrtdiv and spherical_gradient on device tensors are chains of the ops, each link within its bound
    of the host twin applied to what the link was given.  Then the chains against exact identities, each within the sum of its
    links' bounds (the synthesis bound passed through the exact analysis, plus the analysis bound; nothing measured enters):
    vrtdiv(uv(zeta, delta)) = (zeta, delta); curl(grad x) = 0; div(grad x) = the coefficients of the existing spherical_laplacian(x)."""
    from DLWP import ops, verify
    from DLWP.remap import spharm
    rng = np.random.default_rng(31)
    kind, nlat, L = 'gauss', 48, 100
    lat = R.latitudes(kind, nlat)
    tr = _transform(kind, nlat, L)
    T = tr.truncation
    a = 6371200.
    zeta = S.random_packed(rng, T, (2, 3), slope=1.0).astype(np.complex64) * np.float32(1e-5)
    delta = S.random_packed(rng, T, (2, 3), slope=1.0).astype(np.complex64) * np.float32(1e-6)
    zeta[..., 0], delta[..., 0] = 0, 0
    r_uv64, r_a64 = spharm.uv_response(T, a), np.full(T + 1, 1.0 / a)
    r_uv, r_a = r_uv64.astype(np.float32), r_a64.astype(np.float32)
    u, v = verify.spherical_uv(_dev(zeta), _dev(delta), lat, L)
    assert isinstance(u, torch.Tensor) and u.shape == (2, 3, nlat, L) and u.dtype == torch.float32
    cu, cv = ops.spherical_vector_synthesis(_dev(zeta), _dev(delta), tr, _dev(r_uv), _dev(r_uv))
    assert _same_bits(u, cu) and _same_bits(v, cv)
    _check_synthesis((u, v), zeta, delta, r_uv, r_uv, tr, kind, False, 'spherical_uv')
    z2, d2 = verify.spherical_vrtdiv(u, v, lat=lat)
    assert z2.dtype == torch.complex64 and z2.shape == zeta.shape
    uh, vh = u.cpu().numpy().astype(np.float64), v.cpu().numpy().astype(np.float64)
    _check_analysis((z2, d2), uh, vh, r_a, tr, kind, False, 'spherical_vrtdiv')
    # the round trip: the synthesis bound through the exact analysis, plus the analysis bound
    tol = _chain_tolerances(V.analysis_bound(uh, vh, r_a64, kind, T),
                            V.analysis_propagation(*V.synthesis_bound(zeta, delta, r_uv64, r_uv64, kind, nlat, T), r_a64, kind, T),
                            max(np.abs(zeta).max(), np.abs(delta).max()))
    for name, got, ref, lim in (('vrt', z2, zeta, tol[0]), ('div', d2, delta, tol[1])):
        err = _component_error(got.cpu().numpy(), ref.astype(np.complex128))
        print('device round trip vrtdiv(uv(.)), %s: largest error %.3g of the largest coefficient, %.4f of the chain\'s bound'
              % (name, err.max() / np.abs(ref).max(), float((err / np.maximum(lim, TINY)).max())))
        assert (err <= lim).all()
    # the gradient: the vector synthesis of the device's own coefficients
    x = _dev(R.make_field(rng, (2, 3, nlat, L), 'red'))
    gx, gy = verify.spherical_gradient(x, lat=lat)
    assert gx.shape == x.shape and gy.dtype == torch.float32
    coef = ops.spherical_analysis(x, tr).cpu().numpy()
    _check_synthesis((gx, gy), None, coef, None, r_a, tr, kind, False, 'spherical_gradient')
    xp = x.permute(3, 0, 2, 1)
    px, py = verify.spherical_gradient(xp, lat=lat, lat_axis=2, lon_axis=0)
    assert px.shape == xp.shape and _same_bits(px, gx.permute(3, 0, 2, 1)) and _same_bits(py, gy.permute(3, 0, 2, 1))
    gz, gd = verify.spherical_vrtdiv(gx, gy, lat=lat)
    gxh, gyh = gx.cpu().numpy().astype(np.float64), gy.cpu().numpy().astype(np.float64)
    _check_analysis((gz, gd), gxh, gyh, r_a, tr, kind, False, 'vrtdiv of the gradient')
    # curl(grad x) = 0 and div(grad x) = lap x exactly, for the coefficients both chains start from
    r_lap = spharm.laplacian_response(T, a)
    exact = coef.astype(np.complex128) * np.concatenate([r_lap[m:] for m in range(T + 1)])
    scale = np.abs(exact).max()
    tol = _chain_tolerances(V.analysis_bound(gxh, gyh, r_a64, kind, T),
                            V.analysis_propagation(*V.synthesis_bound(None, coef, None, r_a64, kind, nlat, T), r_a64, kind, T), scale)
    curl = _component_error(gz.cpu().numpy(), np.zeros_like(exact))
    print('curl(grad): %.3g of the largest coefficient of the Laplacian, %.4f of the chain\'s bound'
          % (curl.max() / scale, float((curl / np.maximum(tol[0], TINY)).max())))
    assert (curl <= tol[0]).all()
    # the existing call: spherical_laplacian(x) is the scalar synthesis of the same coefficients with -n (n + 1) / a^2; its
    # coefficients come back through the scalar analysis.  Both sides are within their chain's bound of `exact`.
    lap_grid = verify.spherical_laplacian(x, lat=lat)
    assert _same_bits(lap_grid, ops.spherical_synthesis(_dev(coef), tr, _dev(r_lap.astype(np.float32))))
    lap = ops.spherical_analysis(lap_grid, tr).cpu().numpy()
    lh = lap_grid.cpu().numpy().astype(np.float64)
    lap_tol = (S.analysis_bound(lh, kind)[..., None]                      # (a bound of the complex error: it holds for Re and Im)
               + V.scalar_analysis_propagation(S.synthesis_bound(coef, kind, nlat, r_lap), kind, T) + 1e-11 * scale)
    assert (_component_error(lap, exact) <= lap_tol).all()
    diff = _component_error(gd.cpu().numpy(), lap.astype(np.complex128))
    lim = tol[1] + lap_tol
    print('div(grad) - laplacian: %.3g of the largest coefficient, %.4f of the two chains\' bounds'
          % (diff.max() / scale, float((diff / np.maximum(lim, TINY)).max())))
    assert (diff <= lim).all()


def _flux_reference(z, u, v, f):
    s = (f[None, :, None] + z).astype(np.float32)
    return (s * u).astype(np.float32), (s * v).astype(np.float32)


def _update_reference(tend, z, zp, damp, dt, rc, first):
    f32 = np.float32
    parts = lambda c: np.stack([c.real, c.imag]).astype(f32)           # noqa: E731
    t, z, zp, d, dt, rc = parts(tend), parts(z), parts(zp), damp.astype(f32), f32(dt), f32(rc)
    t = ((t - (d * zp).astype(f32)).astype(f32) / (f32(1) + (d * dt).astype(f32)).astype(f32)).astype(f32)
    if first:
        new = (z + (dt * t).astype(f32)).astype(f32)
        zf = (z + (rc * (new - z).astype(f32)).astype(f32)).astype(f32)
    else:
        z1 = (z + (rc * (zp - (f32(2) * z).astype(f32)).astype(f32)).astype(f32)).astype(f32)
        new = (zp + ((f32(2) * dt) * t).astype(f32)).astype(f32)
        zf = (z1 + (rc * new).astype(f32)).astype(f32)
    return (new[0] + 1j * new[1]).astype(np.complex64), (zf[0] + 1j * zf[1]).astype(np.complex64)


@pytest.mark.parametrize('fields,nlat,L', [(1, 2, 12), (33, 19, 37), (5, 33, 72), (70, 48, 100)])
def test_flux_is_its_float32_restatement(fields, nlat, L):
    from DLWP import ops
    rng = np.random.default_rng(fields)
    z, u, v = (rng.standard_normal((fields, nlat, L)).astype(np.float32) for _ in range(3))
    f = rng.standard_normal(nlat).astype(np.float32)
    wf, wg = _flux_reference(z, u, v, f)
    F, G = ops.barotropic_flux(_dev(z), _dev(u), _dev(v), _dev(f))
    assert np.array_equal(F.cpu().numpy().view(np.int32), wf.view(np.int32)) and np.array_equal(G.cpu().numpy().view(np.int32), wg.view(np.int32))
    # one element off a 16-byte line, into given outputs
    off = [torch.zeros(z.size + 1, dtype=torch.float32, device=DEV)[1:].view(z.shape) for _ in range(5)]
    for t, h in zip(off, (z, u, v)):
        t.copy_(torch.from_numpy(h))
    rf, rg = ops.barotropic_flux(off[0], off[1], off[2], _dev(f), off[3], off[4])
    assert rf is off[3] and _same_bits(rf, F) and _same_bits(rg, G)


@pytest.mark.parametrize('fields,T', [(1, 0), (3, 1), (33, 9), (2, 21), (65, 32)])
def test_update_is_its_float32_restatement(fields, T):
    from DLWP import ops
    rng = np.random.default_rng(T)
    rows = S.packed_rows(T)
    mk = lambda: (rng.standard_normal((fields, rows)) + 1j * rng.standard_normal((fields, rows))).astype(np.complex64)     # noqa: E731
    tend, z, zp = mk() * np.float32(1e-3), mk(), mk()
    damp = (rng.random(rows) * 1e-3).astype(np.float32)
    for first in (True, False):
        wz, wp = _update_reference(tend, z, zp, damp, 600., 0.04, first)
        dz, dp = _dev(z), _dev(zp)
        ops.barotropic_update(_dev(tend), dz, dp, _dev(damp), 600., 0.04, first)
        assert np.array_equal(torch.view_as_real(dz).cpu().numpy().view(np.int32), np.stack([wz.real, wz.imag], -1).view(np.int32))
        assert np.array_equal(torch.view_as_real(dp).cpu().numpy().view(np.int32), np.stack([wp.real, wp.imag], -1).view(np.int32))
        # 8 bytes off a 16-byte line: the element path
        offs = []
        for h in (tend, z, zp):
            buf = torch.zeros(fields * rows + 1, dtype=torch.complex64, device=DEV)[1:].view(fields, rows)
            buf.copy_(torch.from_numpy(h))
            offs.append(buf)
        assert offs[1].data_ptr() % 16 == 8
        ops.barotropic_update(offs[0], offs[1], offs[2], _dev(damp), 600., 0.04, first)
        assert _same_bits(offs[1], dz) and _same_bits(offs[2], dp)


def test_first_use_inside_a_capture_is_refused():
    from DLWP import ops
    from DLWP._native import NativeError
    from DLWP.remap import spharm
    tr = spharm.SphericalTransform(R.latitudes('fejer', 22, False), 48)        # a transform no other test has used
    c = torch.zeros((2, S.packed_rows(tr.truncation)), dtype=torch.complex64, device=DEV)
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(NativeError, match='capture'):
        with torch.cuda.graph(graph):
            ops.spherical_vector_synthesis(c, None, tr)
    torch.cuda.synchronize()
    u, v = ops.spherical_vector_synthesis(c, None, tr)
    assert not bool(u.any()) and not bool(v.any())


def test_refusals_on_the_device():
    from DLWP import ops
    tr = _transform('clenshaw-curtis', 17, 36)
    rows = S.packed_rows(tr.truncation)
    x = torch.zeros((2, 17, 36), device=DEV)
    c = torch.zeros((2, rows), dtype=torch.complex64, device=DEV)
    with pytest.raises(ValueError, match='transform is for'):
        ops.spherical_vector_analysis(x[:, :, :32], x[:, :, :32], tr)
    with pytest.raises(ValueError, match='one shape'):
        ops.spherical_vector_analysis(x, x[:1], tr)
    with pytest.raises(TypeError):
        ops.spherical_vector_analysis(x.double(), x, tr)
    with pytest.raises(ValueError, match='response'):
        ops.spherical_vector_analysis(x, x, tr, torch.ones(3, device=DEV))
    with pytest.raises(ValueError, match='one shape'):
        ops.spherical_vector_synthesis(c, c[:1], tr)
    with pytest.raises(ValueError, match='output must'):
        ops.spherical_vector_synthesis(c, None, tr, out_u=torch.zeros((2, 17, 32), device=DEV))
    with pytest.raises(ValueError, match='unit stride'):
        ops.spherical_vector_synthesis(c, None, tr, out_v=torch.zeros((2, 36, 17), device=DEV).permute(0, 2, 1))
    both = torch.zeros((2, 2, 17, 36), device=DEV)
    with pytest.raises(ValueError, match='overlap'):
        ops.spherical_vector_synthesis(c, None, tr, out_u=both[0], out_v=both[0])
    with pytest.raises(ValueError, match='overlap'):
        ops.spherical_vector_synthesis(c, None, tr, out_u=both[:, 0], out_v=both[0])
    iu, iv = ops.spherical_vector_synthesis(c + 1, None, tr, out_u=both[:, 0], out_v=both[:, 1])      # interleaved: apart
    wu, wv = ops.spherical_vector_synthesis(c + 1, None, tr)
    assert _same_bits(iu, wu) and _same_bits(iv, wv)
    with pytest.raises(ValueError, match='overlaps'):
        ops.barotropic_flux(x, x, x, torch.zeros(17, device=DEV), out_f=x)
    with pytest.raises(ValueError, match='tend overlaps'):
        ops.barotropic_update(c, c, c.clone(), torch.zeros(rows, device=DEV), 600., 0.04, True)
    with pytest.raises(ValueError, match='Coriolis'):
        ops.barotropic_flux(x, x, x, torch.zeros(16, device=DEV))
    with pytest.raises(ValueError, match='two buffers'):
        ops.barotropic_update(c.clone(), c, c, torch.zeros(rows, device=DEV), 600., 0.04, True)
    with pytest.raises(ValueError, match='damp'):
        ops.barotropic_update(c, c.clone(), c.clone(), torch.zeros(rows - 1, device=DEV), 600., 0.04, True)
    z, d = ops.spherical_vector_analysis(x[:0], x[:0], tr)
    assert z.shape == (0, rows) and d.shape == (0, rows)
    u, v = ops.spherical_vector_synthesis(c[:0], None, tr)
    assert u.shape == (0, 17, 36)
