"""
dlwpcs_sht_spectrum on the device against the float64 reference of sht_ref.py.

Bound: sht_ref.bound (derived there for the kernel as written, not measured), NaN exactly where the reference has NaN.  Every test
prints the largest fraction of the bound it saw.  Shapes: latitudes around one MFMA k step and the padding to 4, longitudes odd,
a multiple of 4 and beyond one 64-longitude chunk, truncations on and across the 32-degree tile edge, field counts around the
32-field tile, every shape at the largest truncation it allows and at T = 0, the three quadratures and both forms rotating through
the grid.  Guarded, poisoned, exact-size memory from hostile_mem.py.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hostile_mem as H      # noqa: E402
import sht_ref as R          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_TRANSFORMS = {}


def _transform(kind, nlat, L, T=None, south_first=False):
    from DLWP.remap import spharm
    key = (kind, nlat, L, T, south_first)
    if key not in _TRANSFORMS:
        _TRANSFORMS[key] = spharm.SphericalTransform(R.latitudes(kind, nlat, south_first), L, T)
    return _TRANSFORMS[key]


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check(got, ref, lim, what):
    """got (nq, ..., K) float32 against ref within lim; NaN exactly where the reference has NaN.  Returns the largest fraction."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    ok = ~np.isnan(ref)
    if not ok.any():
        return 0.0
    err = np.abs(got - ref)[ok]
    frac = float((err / np.maximum(lim[ok], np.finfo(np.float64).tiny)).max())
    print('%s: largest |error| / bound = %.4f' % (what, frac))
    assert (err <= lim[ok]).all(), '%s: %.3g of the bound' % (what, frac)
    return frac


def _run(tr, f, v=None, reduced=(), **kw):
    from DLWP import ops
    out, cnt = ops.spherical_spectrum(_dev(f), _dev(v), transform=tr, reduced=reduced, counts=True, **kw)
    out, cnt = out.cpu().numpy(), cnt.cpu().numpy()
    return (out[None] if v is None else out), cnt


@pytest.mark.parametrize('L', R.GPU_L)
def test_shape_grid(L):
    rng = np.random.default_rng(L)
    worst, seen = 0.0, 0
    for kind, nlat, LL, T, fields, pair in R.grid_cases():
        if LL != L:
            continue
        seen += 1
        f = R.make_field(rng, (fields, nlat, L))
        v = R.make_field(rng, (fields, nlat, L), 'red') if pair else None
        got, cnt = _run(_transform(kind, nlat, L, T), f, v)
        ref, skipped, lim = R.reference(f, v, kind, T)
        assert not cnt.any() and not skipped.any()
        worst = max(worst, _check(got, ref, lim, '%s %d x %d T=%d fields=%d pair=%d' % (kind, nlat, L, T, fields, pair)))
    assert seen >= len(R.GPU_NLAT)
    print('L = %d: largest fraction of the bound over the grid = %.4f' % (L, worst))


@pytest.mark.parametrize('T', R.GPU_T_EDGE)
def test_truncations_on_and_across_the_degree_tile(T):
    rng = np.random.default_rng(T)
    f, v = R.make_field(rng, (3, 48, 96)), R.make_field(rng, (3, 48, 96), 'red')
    got, _ = _run(_transform('gauss', 48, 96, T), f, v)
    ref, _, lim = R.reference(f, v, 'gauss', T)
    _check(got, ref, lim, 'gauss 48 x 96 T=%d' % T)
    # a smaller truncation is the head of a larger one bit for bit: the orders and degrees beyond it never enter
    more, _ = _run(_transform('gauss', 48, 96, 41), f, v)
    assert _same_bits(more[..., :T + 1], got)


@pytest.mark.parametrize('fields', R.GPU_FIELDS)
def test_field_counts_forms_and_repeatability(fields):
    rng = np.random.default_rng(fields)
    tr = _transform('clenshaw-curtis', 33, 72)
    assert tr.truncation == 16
    f, v = R.make_field(rng, (fields, 33, 72), 'red'), R.make_field(rng, (fields, 33, 72))
    pair, _ = _run(tr, f, v)
    again, _ = _run(tr, f, v)
    single, _ = _run(tr, f)
    other, _ = _run(tr, v)
    assert _same_bits(pair, again), 'two runs of one call differ'
    assert _same_bits(single[0], pair[0]) and _same_bits(other[0], pair[1]), 'the single form is not the pair form\'s power'
    ref, _, lim = R.reference(f, v, 'clenshaw-curtis', 16)
    _check(pair, ref, lim, 'fields=%d' % fields)


def test_leading_dims_permuted_view_and_alignment():
    from DLWP import ops
    rng = np.random.default_rng(7)
    kind, nlat, L = 'fejer', 10, 12
    tr = _transform(kind, nlat, L)
    T = tr.truncation
    f, v = R.make_field(rng, (3, 5, 2, nlat, L)), R.make_field(rng, (3, 5, 2, nlat, L))
    ft, vt = _dev(f), _dev(v)
    for red in ((1,), (0, 2), (0, 1, 2), ()):
        out = ops.spherical_spectrum(ft, vt, transform=tr, reduced=red).cpu().numpy()
        ref, _, lim = R.reference(f, v, kind, T, red)
        _check(out, ref, lim, 'interleaved %r' % (red,))
    # a permuted view: the same numbers seen as (2, nlat, 5, L, 3), the latitude axis second, longitude not last
    fp, vp = ft.permute(2, 3, 1, 4, 0), vt.permute(2, 3, 1, 4, 0)
    outp = ops.spherical_spectrum(fp, vp, transform=tr, lat_axis=1, lon_axis=3, reduced=(2,)).cpu().numpy()
    refp, _, limp = R.reference(f.transpose(2, 1, 0, 3, 4), v.transpose(2, 1, 0, 3, 4), kind, T, (1,))
    _check(outp, refp, limp, 'permuted')
    # a latitude axis that is not second-to-last, longitude unit-stride: no copy is made, the rows lie 4 * L apart
    g = R.make_field(rng, (3, nlat, 4, L))
    gt = _dev(g)
    a = ops.spherical_spectrum(gt, transform=tr, lat_axis=1).cpu().numpy()
    b = ops.spherical_spectrum(_dev(g.transpose(0, 2, 1, 3)), transform=tr).cpu().numpy()
    assert _same_bits(a, b)
    ref, _, lim = R.reference(g.transpose(0, 2, 1, 3), None, kind, T)
    _check(a[None], ref, lim, 'latitude axis in the middle')
    # one element off a 16-byte line: the scalar-load path on the numbers the vector path has just served
    for kind2, nlat2, L2 in (('fejer', 10, 12), ('clenshaw-curtis', 65, 72)):
        tr2 = _transform(kind2, nlat2, L2)
        h = R.make_field(rng, (3, nlat2, L2))
        buf = torch.zeros(h.size + 1, dtype=torch.float32, device=DEV)
        x = buf[1:].view(3, nlat2, L2)
        x.copy_(torch.from_numpy(h))
        assert x.data_ptr() % 16 == 4
        a = ops.spherical_spectrum(x, transform=tr2).cpu().numpy()
        b = ops.spherical_spectrum(_dev(h), transform=tr2).cpu().numpy()
        assert _same_bits(a, b)
        ref, _, lim = R.reference(h, None, kind2, tr2.truncation)
        _check(a[None], ref, lim, 'offset base %d x %d' % (nlat2, L2))
    # latitudes south to north: the table is built in the order of the latitude vector
    trs = _transform(kind, nlat, L, None, True)
    s, _ = _run(trs, f[0, 0, :, ::-1], None)
    n, _ = _run(tr, f[0, 0], None)
    ref, _, lim = R.reference(f[0, 0], None, kind, T)
    _check(s, ref, lim, 'south first')
    _check(n, ref, lim, 'north first')


@pytest.mark.parametrize('pair', [False, True])
def test_missing_fields_are_counted_and_leave_no_trace(pair):
    rng = np.random.default_rng(23 + pair)
    kind, nlat, L, groups, rows = 'clenshaw-curtis', 17, 37, 3, 40
    tr = _transform(kind, nlat, L)
    f = R.make_field(rng, (groups, rows, nlat, L))
    v = R.make_field(rng, (groups, rows, nlat, L)) if pair else None
    gone = [0, 7, 31, 32, 33, rows - 1]
    keep = [r for r in range(rows) if r not in gone]
    fh, vh = f.copy(), (v.copy() if pair else None)
    for n, r in enumerate(gone):                                         # one cell of the field: a NaN payload or an infinity
        for g in range(groups):
            tgt = vh if (pair and n % 2) else fh                         # some fields missing in the verification only
            tgt.view(np.uint32)[g, r, rng.integers(0, nlat), rng.integers(0, L)] = R.NAN_BITS[(n + g) % len(R.NAN_BITS)]
    got, cnt = _run(tr, fh, vh, (1,))
    assert cnt.dtype == np.int32 and (cnt == len(gone)).all()
    ref, skipped, lim = R.reference(fh, vh, kind, tr.truncation, (1,))
    assert (skipped == len(gone)).all()
    _check(got, ref, lim, 'holes pair=%d' % pair)
    assert rows <= 512                                                   # one DLWPCS_GROUP_SLAB_ROWS slab: the identity is bitwise
    cut, cnt2 = _run(tr, f[:, keep], None if v is None else v[:, keep], (1,))
    assert not cnt2.any()
    assert _same_bits(got, cut), 'the means differ from those of the input with the missing fields taken out'
    # per field: NaN rows exactly for the missing fields, the others untouched
    each, flags = _run(tr, fh, vh)
    clean, _ = _run(tr, f, v)
    assert np.array_equal(flags != 0, np.isin(np.arange(rows), gone)[None, :].repeat(groups, 0))
    assert np.isnan(each[:, :, gone]).all() and _same_bits(each[:, :, keep], clean[:, :, keep])
    # a whole group missing: NaN and a full count there, the other groups untouched
    fg = f.copy()
    fg.view(np.uint32)[1, :, 0, 0] = R.NAN_BITS[1]
    one, cnt3 = _run(tr, fg, v, (1,))
    mean, _ = _run(tr, f, v, (1,))
    assert cnt3.tolist() == [0, rows, 0] and np.isnan(one[:, 1]).all()
    assert _same_bits(one[:, [0, 2]], mean[:, [0, 2]])


def test_offset_and_red_fields():
    rng = np.random.default_rng(31)
    for kind, nlat, L in (('clenshaw-curtis', 33, 72), ('gauss', 24, 50), ('fejer', 16, 36)):
        tr = _transform(kind, nlat, L)
        f, v = R.make_field(rng, (3, nlat, L), 'white', 280.0), R.make_field(rng, (3, nlat, L), 'red', 280.0)
        got, _ = _run(tr, f, v)
        ref, _, lim = R.reference(f, v, kind, tr.truncation)
        _check(got, ref, lim, 'offset %s %d x %d' % (kind, nlat, L))


def test_one_degree_grid():
    """clenshaw-curtis 181 x 360 at T = 90, two fields, the pair form"""
    rng = np.random.default_rng(41)
    tr = _transform('clenshaw-curtis', 181, 360)
    assert tr.truncation == 90
    f, v = R.make_field(rng, (2, 181, 360), 'red', 280.0), R.make_field(rng, (2, 181, 360))
    got, cnt = _run(tr, f, v)
    ref, _, lim = R.reference(f, v, 'clenshaw-curtis', 90)
    assert not cnt.any()
    _check(got, ref, lim, '181 x 360 T=90')


@pytest.mark.parametrize('kind,nlat,L,T,fields,pair', [('clenshaw-curtis', 17, 37, 8, 33, True), ('gauss', 48, 96, 40, 3, False),
                                                       ('fejer', 65, 130, 32, 5, True)])
def test_guarded_memory(monkeypatch, kind, nlat, L, T, fields, pair):
    """inputs, scratch and outputs in exact-size, poisoned, guarded allocations: nothing outside them is written, every element
    of the output is"""
    from DLWP import ops
    rng = np.random.default_rng(nlat + L)
    arena = H.Arena(96 << 20, DEV)
    hw = H.hostile_workspaces(monkeypatch, device=DEV, arena=arena)
    tr = _transform(kind, nlat, L, T)
    f = R.make_field(rng, (fields, nlat, L))
    v = R.make_field(rng, (fields, nlat, L)) if pair else None
    ft = arena.place(torch.from_numpy(f).to(DEV), 'f')
    vt = arena.place(torch.from_numpy(v).to(DEV), 'v') if pair else None
    out = arena.tensor(((3,) if pair else ()) + (fields, T + 1), torch.float32, 'out')
    flags = arena.tensor((fields,), torch.int32, 'skipped')
    twiddle, table = tr.device_tables(DEV)                               # (the tables are not scratch: made before the poisoning)
    d = ops.sht_desc(nlat, L, T, ops.spectrum_dims((fields,), [(nlat * L,), (nlat * L,) if pair else (0,)], ()), (L, L if pair else 0))
    ops.sht_launch(d, ft, vt, twiddle, table, out, flags)
    hw.check()
    assert hw.requests and hw.requests[-1][0] == 'sht'
    assert not bool(H.is_poison(out).any()) and not bool(H.is_poison(flags).any())
    assert int(flags.abs().sum()) == 0
    got = out.cpu().numpy()
    ref, _, lim = R.reference(f, v, kind, T)
    _check(got if pair else got[None], ref, lim, 'guarded %d x %d' % (nlat, L))
    want, _ = _run(tr, f, v)
    assert _same_bits(got if pair else got[None], want)


def test_graph_capture():
    from DLWP import ops
    from DLWP._native import NativeError
    from DLWP.remap import spharm
    rng = np.random.default_rng(43)
    kind, nlat, L = 'clenshaw-curtis', 17, 36
    f, v = _dev(R.make_field(rng, (4, 6, nlat, L))), _dev(R.make_field(rng, (4, 6, nlat, L)))
    fresh = spharm.SphericalTransform(R.latitudes(kind, nlat), L)        # never used on the device
    graph0 = torch.cuda.CUDAGraph()
    with pytest.raises(NativeError, match='capture'):
        with torch.cuda.graph(graph0):
            ops.spherical_spectrum(f, v, transform=fresh, reduced=(1,))
    torch.cuda.synchronize()
    eager, cnt = ops.spherical_spectrum(f, v, transform=fresh, reduced=(1,), counts=True)
    eager, cnt = eager.clone(), cnt.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.spherical_spectrum(f, v, transform=fresh, reduced=(1,), counts=True)      # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                        # one stream: a single chain of launches
        res, rcnt = ops.spherical_spectrum(f, v, transform=fresh, reduced=(1,), counts=True)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(res.view(torch.int32), eager.view(torch.int32)) and torch.equal(rcnt, cnt)
    ref, _, lim = R.reference(f.cpu().numpy(), v.cpu().numpy(), kind, fresh.truncation, (1,))
    _check(res.cpu().numpy(), ref, lim, 'graph replay')
    # new data in the captured input: the replay follows it
    f.copy_(v)
    graph.replay()
    torch.cuda.synchronize()
    again = res.cpu().numpy()
    assert _same_bits(again[0], again[1])


def test_refusals_on_the_device():
    from DLWP import ops
    tr = _transform('clenshaw-curtis', 17, 36)
    x = torch.zeros((2, 17, 36), device=DEV)
    with pytest.raises(ValueError, match='transform is for'):
        ops.spherical_spectrum(x[:, :, :32], transform=tr)
    with pytest.raises(ValueError, match='grid axis'):
        ops.spherical_spectrum(x, transform=tr, reduced=(1,))
    with pytest.raises(TypeError):
        ops.spherical_spectrum(x.double(), transform=tr)
    with pytest.raises(TypeError):
        ops.spherical_spectrum(x)


def test_cube_to_latlon_to_spherical_spectrum():
    """a C12 cube field -> inverse_remap_array onto a 10-degree grid of cell centres ('fejer') -> verify on device tensors,
    compared with the host path on the downloaded arrays"""
    from DLWP import verify
    from DLWP.remap import CubeSphereGrid, CubeSphereRemap, LatLonGrid
    cube, ll = CubeSphereGrid(12), LatLonGrid.cells(18, 36, inverse_lat=False, lon_begin=0.)
    r = CubeSphereRemap(verbose=False)
    r.generate_maps(grid=cube, latlon=ll, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn((6, 4) + tuple(cube.shape), generator=g, device=DEV)
    f = r.inverse_remap_array(x)
    assert tuple(f.shape) == (6, 4, 18, 36)
    v = torch.roll(f, 3, dims=-1) + 0.5 * torch.randn(f.shape, generator=g, device=DEV)
    lat = -85. + 10. * np.arange(18)
    cd, cnt = verify.spherical_cross_spectrum(f, v, lat=lat, axis=0, return_count=True)
    ch = verify.spherical_cross_spectrum(f.cpu().numpy(), v.cpu().numpy(), lat=lat, axis=0)
    assert cd.power_f.shape == (4, 9) and cd.power_f.dtype == np.float64 and not cnt.any()
    ref, _, lim = R.reference(f.cpu().numpy(), v.cpu().numpy(), 'fejer', 8, (0,), south_first=True)
    _check(np.stack(cd), ref, lim, 'end to end')
    assert np.abs(np.stack(ch) - ref).max() <= 1e-12 * np.abs(ref).max()
    dev = verify.spherical_correlation(f, v, lat=lat)
    host = verify.spherical_correlation(f.cpu().numpy(), v.cpu().numpy(), lat=lat)
    assert dev.shape == (9,) and np.abs(dev - host).max() <= 1e-3 and (np.abs(dev) <= 1 + 1e-5).all()
    one = verify.spherical_spectrum(f, lat=lat, axis=(0, 1), truncation=5)
    assert one.shape == (6,) and np.abs(one - verify.spherical_spectrum(f.cpu().numpy(), lat=lat, truncation=5)).max() <= lim[0].max()
