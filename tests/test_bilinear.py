"""
CPU tests of the bilinear sampling map (DLWP/remap/bilinear.py, the host twin of csrc/bilinear.hip): the dual mesh, the weights
against points whose face and weights are known by construction, the properties every answer must have, continuity across a cube
edge and a cube vertex, second-order convergence, invariance under the grid's rotation, and the map / forecast interface.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bilinear_cases as bc   # noqa: E402

NAMES = sorted(bc.CUBES)


@pytest.mark.parametrize('N', [1, 2, 3, 5, 8])
def test_dual_mesh_is_a_closed_surface(N):
    from DLWP.remap import CubeSphereGrid, dual_faces
    quads, tris = dual_faces(CubeSphereGrid(N))
    assert quads.shape == (6 * (N - 1) ** 2 + 12 * (N - 1), 4) and tris.shape == (8, 3)
    F = quads.shape[0] + tris.shape[0]
    assert F == 6 * (N - 1) ** 2 + 12 * (N - 1) + 8
    sides = {}
    for faces in (quads, tris):
        for fc in faces:
            assert len(set(fc.tolist())) == len(fc)
            for k in range(len(fc)):
                key = tuple(sorted((int(fc[k]), int(fc[(k + 1) % len(fc)]))))
                sides[key] = sides.get(key, 0) + 1
    assert set(sides.values()) == {2}                               # every side is shared by exactly two faces
    V = len(set(quads.ravel().tolist()) | set(tris.ravel().tolist()))
    assert V == 6 * N * N
    assert V - len(sides) + F == 2                                  # Euler


def test_cube_topology_is_an_involution():
    from DLWP.remap.bilinear import cube_edges
    e = cube_edges()
    assert e.shape == (6, 4, 3) and e.dtype == np.int32
    for f in range(6):
        for s in range(4):
            g, t, rev = e[f, s]
            assert g != f and tuple(e[g, t]) == (f, s, rev)
    assert sorted(e[..., 0].ravel().tolist()) == sorted(list(range(6)) * 4)


@pytest.mark.parametrize('name', NAMES)
def test_points_made_inside_a_face_get_its_cells_and_weights(name):
    lat, lon, cells, w_made = bc.interior(name)
    col, w = bc.host_weights(name, 'interior')
    assert col.dtype == np.int32 and w.dtype == np.float64 and col.shape == w.shape == (lat.size, 4)
    tri = cells[:, 3] < 0
    assert np.array_equal(np.sort(col[~tri], axis=1), np.sort(cells[~tri], axis=1))
    assert np.array_equal(np.sort(col[tri, :3], axis=1), np.sort(cells[tri, :3], axis=1))
    assert np.array_equal(col[tri, 3], col[tri, 2])
    # the weight the twin gives to each generating cell
    got = (w[:, None, :] * (col[:, None, :] == cells[:, :, None])).sum(axis=2)
    got[tri, 3] = w[tri, 3]
    assert np.abs(got - w_made).max() <= 1e-12


@pytest.mark.parametrize('name', NAMES)
def test_properties_of_every_answer(name):
    cb = bc.cube(name)
    lat, lon = bc.interior(name)[:2]
    col, w = bc.host_weights(name, 'interior')
    bc.check_properties(cb, lat, lon, col, w)
    lat, lon, own = bc.boundary(name)
    col, w = bc.host_weights(name, 'boundary')
    bc.check_properties(cb, lat, lon, col, w, own)


@pytest.mark.parametrize('through', ['edge', 'vertex'])
def test_the_sampled_field_is_continuous_across_edges_and_corners(through):
    """2000 steps round a great circle that crosses a cube edge obliquely at its middle, or passes through a cube vertex, on
    N = 5.  The field x y + z has the Lipschitz constant sqrt(2) on the sphere; its interpolant on well-shaped cells cannot
    move faster than a small multiple of that, taken as 4 (derived, not measured).  A sampler that kinks at the cube's edges
    jumps there by O(h^2) with h = pi / 10, far more than the bound for one step of 2 pi / 2000 (0.018)."""
    from DLWP.remap import point_weights
    cb = bc.cube('N5')
    p = np.array([1., 1., 0.]) / np.sqrt(2.) if through == 'edge' else np.array([1., 1., 1.]) / np.sqrt(3.)
    q = np.cross(p, np.array([0.3, -0.5, 0.81]))
    q /= np.linalg.norm(q)
    th = 2 * np.pi * np.arange(2001) / 2000
    pts = np.cos(th)[:, None] * p + np.sin(th)[:, None] * q
    lat, lon = bc.latlon_of(pts)
    col, w = point_weights(cb, lat, lon)
    v = bc.sample(cb, col, w)
    step = 2 * np.pi / 2000
    assert np.abs(np.diff(v)).max() <= 4 * bc.LIPSCHITZ * step
    assert abs(v[0] - v[-1]) <= 1e-12


def _containing_cell(cb, P):
    N = cb.N
    f = np.argmax(P @ cb.frames[:, 0].T, axis=1)
    fr = cb.frames[f]
    p0 = np.einsum('nk,nk->n', P, fr[:, 0])
    a = (np.arctan2(np.einsum('nk,nk->n', P, fr[:, 1]), p0) + np.pi / 4) / (np.pi / (2 * N))
    b = (np.arctan2(np.einsum('nk,nk->n', P, fr[:, 2]), p0) + np.pi / 4) / (np.pi / (2 * N))
    return (f * N + np.clip(np.floor(b), 0, N - 1).astype(np.int64)) * N + np.clip(np.floor(a), 0, N - 1).astype(np.int64)


def test_second_order_and_better_than_piecewise_constant():
    """Max error of sampling x y + z at 5000 seeded points for N = 8, 16, 32.  Taylor gives a ratio of 4 per doubling; at least
    3 is asserted for both doublings (the twin measures 3.70 and 4.03).  At each N the error is below that of the first-order
    conservative inverse map on a fine grid, which hands every point the value of the cube cell it lies in."""
    from DLWP.remap import CubeSphereGrid, point_weights
    rng = np.random.default_rng(5)
    P = rng.standard_normal((5000, 3))
    P /= np.linalg.norm(P, axis=1, keepdims=True)
    lat, lon = bc.latlon_of(P)
    P = bc.unit(lat, lon)
    errs = []
    for N in (8, 16, 32):
        cb = CubeSphereGrid(N)
        col, w = point_weights(cb, lat, lon)
        err = float(np.abs(bc.sample(cb, col, w) - bc.field(P)).max())
        const = float(np.abs(bc.field(cb.centres.reshape(-1, 3))[_containing_cell(cb, P)] - bc.field(P)).max())
        print('N = %d: bilinear %.3g, piecewise constant %.3g' % (N, err, const))
        assert err < const
        errs.append(err)
    print('ratios %.3f, %.3f' % (errs[0] / errs[1], errs[1] / errs[2]))
    assert errs[0] / errs[1] >= 3. and errs[1] / errs[2] >= 3.


def test_rotation_of_the_grid_does_not_change_the_weights():
    from DLWP.remap import point_weights
    lat, lon = bc.interior('N5_mirrored')[:2]
    col, w = bc.host_weights('N5_mirrored', 'interior')
    back = bc.unit(lat, lon) @ bc.rotation()                        # R^T p: the same points on the default grid
    col0, w0 = point_weights(bc.cube('N5'), *bc.latlon_of(back))
    assert np.array_equal(col, col0)
    assert np.abs(w - w0).max() <= 1e-12


def test_longitudes_wrap_and_shapes_flatten():
    from DLWP.remap import point_weights
    cb = bc.cube('N3')
    lat = np.array([[10., -40.], [77., 0.]])
    lon = np.array([[12., 200.], [359., 0.]])
    col, w = point_weights(cb, lat, lon)
    assert col.shape == (4, 4)
    for shift in (360., -720., 3600.):
        c2, w2 = point_weights(cb, lat.ravel(), lon.ravel() + shift)
        assert np.array_equal(col, c2) and np.abs(w - w2).max() <= 1e-12


def test_value_errors():
    from DLWP.remap import bilinear_map, point_weights
    cb = bc.cube('N3')
    for lat, lon in (([91.], [0.]), ([-90.0001], [0.]), ([np.nan], [0.]), ([0.], [np.inf]), ([0., 1.], [0.])):
        with pytest.raises(ValueError):
            point_weights(cb, lat, lon)
    with pytest.raises(ValueError):
        bilinear_map(cb)
    with pytest.raises(ValueError):
        bilinear_map(cb, [0.], None)


@pytest.mark.parametrize('n', [24, 54])
def test_a_point_list_of_cube_size_stays_a_point_list(n):
    from DLWP.remap import OfflineMap, bilinear_map
    cb = bc.cube('N3')
    rng = np.random.default_rng(n)
    lat, lon = rng.uniform(-90, 90, n), rng.uniform(-180, 540, n)
    m = bilinear_map(cb, lat, lon)
    assert m.dst_kind == 'cells' and m.dst_shape == (n,) and m.src_kind == 'cube' and m.src_shape == (6, 3, 3)
    assert np.array_equal(m.yc_b, lat) and np.array_equal(m.xc_b, lon)
    assert m.nnz == 4 * n and np.array_equal(m.row_ptr, 4 * np.arange(n + 1))
    x = rng.standard_normal((2, 6, 3, 3, 5))
    y = m.apply(x, (1, 2, 3))
    assert y.shape == (2, n, 5)
    col, w = m.col.reshape(n, 4), m.val64.reshape(n, 4)
    assert np.abs(y - np.einsum('nk,bnkc->bnc', w, x.reshape(2, 54, 5)[:, col])).max() <= 1e-14
    # the keyword's default keeps what a rank-1 destination of 6 s^2 cells has always been: a cube
    old = OfflineMap([1], [1], [1.], 54, n, dst_grid_dims=[n])
    assert old.dst_kind == 'cube'
    assert OfflineMap([1], [1], [1.], 54, n, dst_grid_dims=[n], dst_cells=True).dst_kind == 'cells'


def _forecast(cb, rng, dims=('x0', 'x1', 'x2')):
    from DLWP.model.extensions import Forecast
    vals = rng.standard_normal((3, 2) + cb.shape + (2,))
    return Forecast(vals, ('f_hour', 'time') + dims + ('varlev',),
                    {'f_hour': np.arange(3) * 6, 'time': np.arange(2), 'varlev': np.array(['a', 'b'])})


def test_latlon_destination_drives_inverse_remap_forecast(tmp_path):
    from DLWP.remap import CubeSphereRemap, LatLonGrid, bilinear_map, point_weights, read_offline_map, write_offline_map
    cb = bc.cube('N5')
    ll = LatLonGrid.cells(9, 16)
    m = bilinear_map(cb, latlon=ll)
    assert m.dst_kind == 'latlon' and m.dst_shape == (9, 16)
    assert np.array_equal(m.lat_b, ll.lat) and np.array_equal(m.lon_b, ll.lon)
    rng = np.random.default_rng(2)
    fc = _forecast(cb, rng)
    r = CubeSphereRemap(verbose=False)
    r.assign_maps(inverse_map_name=m)
    out = r.inverse_remap_forecast(fc)
    assert out.dims == ('f_hour', 'time', 'lat', 'lon', 'varlev') and out.values.shape == (3, 2, 9, 16, 2)
    assert np.array_equal(out.coords['lat'], ll.lat)
    yc, xc = np.meshgrid(ll.lat, ll.lon, indexing='ij')
    col, w = point_weights(cb, yc, xc)
    want = np.einsum('nk,abnkc->abnc', w, fc.values.reshape(3, 2, -1, 2)[:, :, col]).reshape(3, 2, 9, 16, 2)
    assert np.abs(out.values - want).max() <= 1e-14
    # a file round trip reproduces the map
    path = str(tmp_path / 'sample.nc')
    write_offline_map(m, path)
    back = read_offline_map(path)
    assert np.array_equal(back.row_ptr, m.row_ptr) and np.array_equal(back.col, m.col) and np.array_equal(back.val64, m.val64)
    assert back.dst_kind == 'latlon' and back.dst_shape == (9, 16)


def test_generate_sampling_map_sample_array_and_forecast(tmp_path):
    from DLWP.remap import CubeSphereRemap, LatLonGrid, read_offline_map
    cb = bc.cube('N5')
    rng = np.random.default_rng(3)
    lat, lon = rng.uniform(-90, 90, 7), rng.uniform(0, 360, 7)
    r = CubeSphereRemap(verbose=False)
    with pytest.raises(ValueError):
        r.sample_array(np.zeros(cb.shape))
    with pytest.raises(ValueError):
        r.generate_sampling_map(lat, lon)
    path = str(tmp_path / 'points.nc')
    m = r.generate_sampling_map(lat, lon, res=5, map_name=path)
    assert r.sampling_map is m and m.dst_kind == 'cells'
    back = read_offline_map(path)
    assert np.array_equal(back.row_ptr, m.row_ptr) and np.array_equal(back.col, m.col) and np.array_equal(back.val64, m.val64)
    # a field that is linear in (x, y, z) is reproduced to second order; a constant exactly
    assert np.abs(r.sample_array(np.full(cb.shape, 2.5)) - 2.5).max() <= 1e-14
    x = rng.standard_normal((4,) + cb.shape)
    assert r.sample_array(x).shape == (4, 7)
    assert r.sample_array(np.moveaxis(x, 0, -1), axes=(0, 1, 2)).shape == (7, 4)
    for dims in (('x0', 'x1', 'x2'), ('face', 'height', 'width')):
        fc = _forecast(cb, rng, dims)
        out = r.sample_forecast(fc)
        assert out.dims == ('f_hour', 'time', 'point', 'varlev') and out.values.shape == (3, 2, 7, 2)
        assert np.array_equal(out.coords['lat'], lat) and np.array_equal(out.coords['lon'], lon)
        assert out.lat.dims == ('point',) and out.lon.dims == ('point',)
        assert np.array_equal(out.coords['f_hour'], fc.coords['f_hour'])
        assert np.array_equal(out.values, m.apply(fc.values, (2, 3, 4)))
    # a lat-lon sampling map gives what inverse_remap_forecast gives, and leaves the conservative maps alone
    fwd, inv = r.generate_maps(9, 16, 5)
    assert r.sampling_map is m
    g = r.generate_sampling_map(latlon=LatLonGrid.cells(18, 32))
    out = r.sample_forecast(fc)
    assert out.dims == ('f_hour', 'time', 'lat', 'lon', 'varlev') and out.values.shape == (3, 2, 18, 32, 2)
    assert out.lat.dims == ('lat',) and np.array_equal(out.coords['lon'], g.lon_b)
    assert r.inverse_remap_forecast(fc).values.shape == (3, 2, 9, 16, 2)
    with pytest.raises(ValueError):
        from DLWP.model.extensions import Forecast
        r.sample_forecast(Forecast(np.zeros((2, 3)), ('a', 'b'), {}))
