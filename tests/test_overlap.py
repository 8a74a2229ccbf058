"""
Conservative map generation on the host (DLWP.remap.overlap, the numpy twin of csrc/overlap.hip): entry counts, marginals, an
independent sampled pattern, geography, the two maps, CubeSphereRemap.generate_maps and the map file writer.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import overlap_cases as oc   # noqa: E402

from DLWP.remap import (CubeSphereGrid, CubeSphereRemap, LatLonGrid, conservative_maps, overlap_areas,   # noqa: E402
                        read_offline_map, write_offline_map)

NAMES = sorted(oc.CASES)


@pytest.mark.parametrize('name', NAMES)
def test_counts_signs_and_marginals(name):
    cube, ll = oc.grids(name)
    row_ptr, col, area = oc.host_overlap(name)
    assert area.size == oc.CASES[name][2] == row_ptr[-1]
    assert (area > 0).all()
    for r in range(ll.n_cells):                                  # entries ascend by cube cell within a row
        assert np.all(np.diff(col[row_ptr[r]:row_ptr[r + 1]]) > 0)
    res_ll, res_cs = oc.marginal_residuals(cube, ll, row_ptr, col, area)
    print('%s: marginal residuals %.3g (lat-lon side), %.3g (cube side)' % (name, res_ll, res_cs))
    assert res_ll <= 1e-12 and res_cs <= 1e-12
    assert abs(area.sum() / (4 * np.pi) - 1.) <= 1e-12


def test_inverse_lat_is_the_rows_reversed():
    cube, ll = oc.grids('D')
    n_lat, n_lon = ll.shape

    def dense(name):
        row_ptr, col, area = oc.host_overlap(name)
        D = np.zeros((ll.n_cells, cube.n_cells))
        D[oc.rows_of(row_ptr), col] = area
        return D.reshape(n_lat, n_lon, -1)
    a, b = dense('D'), dense('D_inverse')[::-1]
    assert np.array_equal(a > 0, b > 0)
    assert np.abs(a - b).max() <= 1e-13 * a.max()
    assert np.abs(a[a > 0] / b[a > 0] - 1.).max() <= 1e-13


def _sampled(cube, ll, s=32):
    """(lat-lon cell, cube cell) -> fraction of the cell's s x s sample points (even in longitude and sin latitude) in it"""
    N = cube.N
    off = (np.arange(s) + 0.5) / s
    sl, lo = ll.sin_lat_edges, ll.lon_edges_rad
    sv = (sl[:-1, None] + off[None, :] * np.diff(sl)[:, None]).ravel()            # (n_lat * s)
    lv = (lo[:-1, None] + off[None, :] * np.diff(lo)[:, None]).ravel()            # (n_lon * s)
    S, L = np.meshgrid(sv, lv, indexing='ij')
    cphi = np.sqrt(1. - S * S)
    p = np.stack([cphi * np.cos(L), cphi * np.sin(L), S], axis=-1).reshape(-1, 3)
    d = p @ cube.frames[:, 0].T
    f = np.argmax(d, axis=1)
    dc = d[np.arange(p.shape[0]), f]
    u = np.einsum('nk,nk->n', p, cube.frames[f, 1]) / dc
    v = np.einsum('nk,nk->n', p, cube.frames[f, 2]) / dc
    h = np.pi / (2 * N)
    j = np.clip(np.floor((np.arctan(u) + np.pi / 4) / h), 0, N - 1).astype(np.int64)
    i = np.clip(np.floor((np.arctan(v) + np.pi / 4) / h), 0, N - 1).astype(np.int64)
    c = (f * N + i) * N + j
    ri, rj = np.meshgrid(np.repeat(np.arange(ll.n_lat), s), np.repeat(np.arange(ll.n_lon), s), indexing='ij')
    r = (ri * ll.n_lon + rj).ravel()
    key, cnt = np.unique(r * cube.n_cells + c, return_counts=True)
    return key, cnt / float(s * s)


@pytest.mark.parametrize('name', NAMES)
def test_pattern_against_sampling(name):
    """independent of the closed form: every pair a sample point hits is an entry, and an entry's area is the sampled
    fraction of the lat-lon cell to within 16 / 32 of it (four arcs, each crossing at most 2 * 32 sub-cells per piece)"""
    cube, ll = oc.grids(name)
    row_ptr, col, area = oc.host_overlap(name)
    key, frac = _sampled(cube, ll)
    mine = oc.rows_of(row_ptr) * cube.n_cells + col
    assert np.isin(key, mine).all()
    sampled = np.zeros(mine.size)
    sampled[np.searchsorted(mine, key)] = frac
    ar = ll.area.ravel()[oc.rows_of(row_ptr)]
    assert np.abs(area / ar - sampled).max() <= 16. / 32.


def _maps(name):
    cube, ll = oc.grids(name)
    return conservative_maps(cube, ll)


def test_geography():
    forward, _ = _maps('A')
    oc.check_geography(lambda x: forward.apply_host(x, (0, 1)))


@pytest.mark.parametrize('name', NAMES)
def test_maps_are_normalised_and_conservative(name):
    cube, ll = oc.grids(name)
    forward, inverse = _maps(name)
    assert forward.src_shape == ll.shape and forward.dst_shape == cube.shape and forward.dst_kind == 'cube'
    assert inverse.src_shape == cube.shape and inverse.dst_shape == ll.shape and inverse.dst_kind == 'latlon'
    assert np.array_equal(inverse.lat_b, ll.lat) and np.array_equal(inverse.lon_b, ll.lon)
    assert np.array_equal(forward.yc_b, cube.lat.ravel()) and np.array_equal(forward.xc_b, cube.lon.ravel())
    rng = np.random.default_rng(3)
    for m in (forward, inverse):
        rows = np.bincount(oc.rows_of(m.row_ptr.astype(np.int64)), m.val64, m.n_b)
        assert np.abs(rows - 1.).max() <= 1e-12
        assert np.abs(m.frac_b - 1.).max() <= 1e-12
        assert np.all(np.diff(m.col[m.row_ptr[0]:m.row_ptr[1]]) > 0)
        x = rng.standard_normal(m.src_shape)
        y = m.apply_host(x, tuple(range(x.ndim)))
        a, b = float((m.area_a * x.ravel()).sum()), float((m.area_b * y.ravel()).sum())
        print('%s %s: sum area x = %.17g, remapped %.17g' % (name, m.name, a, b))
        assert abs(a - b) <= 1e-12 * abs(a)


def test_generate_maps_assigns_and_takes_grid_objects(tmp_path):
    cube, ll = oc.grids('B')
    a = CubeSphereRemap(verbose=False)
    fwd, inv = a.generate_maps(5, 8, 3, lon_begin=-7.)
    assert a.cube_grid.N == 3 and a.latlon_grid.shape == (5, 8)
    x = np.full((2, 5, 8), 2.5)
    y = a.remap_array(x)
    assert y.shape == (2, 6, 3, 3) and np.abs(y - 2.5).max() <= 1e-12
    z = a.inverse_remap_array(y)
    assert z.shape == (2, 5, 8) and np.abs(z - 2.5).max() <= 1e-12
    b = CubeSphereRemap(verbose=False)
    fwd2, inv2 = b.generate_maps(grid=cube, latlon=ll)
    for m, n in ((fwd, fwd2), (inv, inv2)):
        assert np.array_equal(m.row_ptr, n.row_ptr) and np.array_equal(m.col, n.col) and np.array_equal(m.val64, n.val64)
    with pytest.raises(ValueError):
        CubeSphereRemap(verbose=False).generate_maps(5, 8)
    with pytest.raises(NotImplementedError):
        a.generate_offline_maps('in.nc', 'out.nc')


@pytest.mark.parametrize('name', ['C', 'D_inverse'])
def test_written_maps_read_back_identical(tmp_path, name):
    cube, ll = oc.grids(name)
    r = CubeSphereRemap(verbose=False)
    paths = str(tmp_path / 'fwd.nc'), str(tmp_path / 'inv.nc')
    made = r.generate_maps(grid=cube, latlon=ll, map_name=paths[0], inverse_map_name=paths[1])
    for m, path in zip(made, paths):
        back = read_offline_map(path)
        assert (back.n_a, back.n_b, back.nnz) == (m.n_a, m.n_b, m.nnz)
        assert back.src_shape == m.src_shape and back.dst_shape == m.dst_shape
        assert back.src_kind == m.src_kind and back.dst_kind == m.dst_kind
        for attr in ('row_ptr', 'col', 'val64', 'val', 'yc_a', 'xc_a', 'yc_b', 'xc_b', 'area_a', 'area_b', 'frac_b'):
            assert np.array_equal(getattr(back, attr), getattr(m, attr)), attr
    assert np.array_equal(read_offline_map(paths[1]).lat_b, ll.lat)
    # a CubeSphereRemap pointed at the files does what the one that made them does
    other = CubeSphereRemap(verbose=False)
    other.assign_maps(*paths)
    x = np.random.default_rng(1).standard_normal(ll.shape)
    assert np.array_equal(other.remap_array(x), r.remap_array(x))


def test_rotated_grid_keeps_the_identities():
    """a rotated and mirrored cube against lat-lon cells: no plane holds the z axis, every bound is a curve"""
    rng = np.random.default_rng(11)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) > 0:
        q[:, 0] = -q[:, 0]
    cube, ll = CubeSphereGrid(5, rotation=q), LatLonGrid.cells(7, 10, lon_begin=4.)
    row_ptr, col, area = overlap_areas(cube, ll)
    res = oc.marginal_residuals(cube, ll, row_ptr, col, area)
    assert (area > 0).all() and max(res) <= 1e-12
