"""
Conservative map generation on the device (dlwpcs_overlap_count / dlwpcs_overlap_fill, csrc/overlap.hip): the kernels against
the numpy twin on the small grids, the marginal identities at larger ones, repeatability, and CubeSphereRemap.generate_maps
with device tensors remapped by the maps it made.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import overlap_cases as oc   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _device_overlap(cube, ll):
    from DLWP import ops
    from DLWP.remap.overlap import DUST
    out = ops.overlap_csr(cube, ll, DUST, DEV)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('name', sorted(oc.CASES))
def test_kernels_against_the_host_twin(name):
    cube, ll = oc.grids(name)
    first = _device_overlap(cube, ll)
    row_ptr, col, area = (t.cpu().numpy() for t in first)
    h_ptr, h_col, h_area = oc.host_overlap(name)
    assert area.size == oc.CASES[name][2]
    assert row_ptr.dtype == np.int64 and col.dtype == np.int32 and area.dtype == np.float64
    assert np.array_equal(row_ptr, h_ptr) and np.array_equal(col, h_col)
    r = oc.rows_of(row_ptr)
    small = np.minimum(ll.area.ravel()[r], cube.area.ravel()[col])
    diff = float((np.abs(area - h_area) / small).max())
    res = oc.marginal_residuals(cube, ll, row_ptr, col, area)
    print('%s: device - host %.3g of the smaller cell; marginal residuals %.3g / %.3g' % ((name, diff) + res))
    assert diff <= 1e-12
    assert (area > 0).all() and max(res) <= 1e-12
    second = _device_overlap(cube, ll)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


def test_identities_c24():
    from DLWP.remap import CubeSphereGrid, LatLonGrid
    cube, ll = CubeSphereGrid(24), LatLonGrid.cells(45, 90, lon_begin=-2.)
    row_ptr, col, area = (t.cpu().numpy() for t in _device_overlap(cube, ll))
    res = oc.marginal_residuals(cube, ll, row_ptr, col, area)
    print('C24 against 45 x 90: %d entries, marginal residuals %.3g (lat-lon side), %.3g (cube side)' % ((area.size,) + res))
    assert (area > 0).all() and max(res) <= 1e-10


def test_identities_c48_pole_centred():
    """181 x 360 with centres on the poles -> C48.  The bound is derived: the maps store fp32 weights (2^-24 = 6e-8), a residual
    below 1e-8 cannot show in a remapped field."""
    from DLWP.remap import CubeSphereGrid, LatLonGrid
    cube, ll = CubeSphereGrid(48), LatLonGrid.from_centres(np.linspace(-90., 90., 181), np.arange(360.))
    row_ptr, col, area = (t.cpu().numpy() for t in _device_overlap(cube, ll))
    res = oc.marginal_residuals(cube, ll, row_ptr, col, area)
    print('C48 against 181 x 360: %d entries, marginal residuals %.3g (lat-lon side), %.3g (cube side)' % ((area.size,) + res))
    assert (area > 0).all() and max(res) <= 1e-8
    for k in range(0, ll.n_cells, 997):
        assert np.all(np.diff(col[row_ptr[k]:row_ptr[k + 1]]) > 0)


def test_rotated_mirrored_cube_matches_host():
    from DLWP.remap import CubeSphereGrid, LatLonGrid, overlap_areas
    rng = np.random.default_rng(11)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) > 0:
        q[:, 0] = -q[:, 0]
    cube, ll = CubeSphereGrid(5, rotation=q), LatLonGrid.cells(7, 10, lon_begin=4.)
    row_ptr, col, area = (t.cpu().numpy() for t in _device_overlap(cube, ll))
    h_ptr, h_col, h_area = overlap_areas(cube, ll)
    assert np.array_equal(row_ptr, h_ptr) and np.array_equal(col, h_col)
    small = np.minimum(ll.area.ravel()[oc.rows_of(row_ptr)], cube.area.ravel()[col])
    assert (np.abs(area - h_area) / small).max() <= 1e-12
    assert max(oc.marginal_residuals(cube, ll, row_ptr, col, area)) <= 1e-12


def test_abi_refuses_bad_descriptors_and_fill_stays_inside():
    from DLWP import _native as nat
    cube, ll = oc.grids('B')
    lib = nat.lib()
    d = nat.OverlapDesc()
    d.N, d.n_lat, d.n_lon, d.dust = 3, 5, 8, 1e-10
    fr = np.ascontiguousarray(cube.frames)
    ctypes.memmove(ctypes.addressof(d.frames), fr.ctypes.data, fr.nbytes)
    sl = torch.from_numpy(ll.sin_lat_edges.copy()).to(DEV)
    lo = torch.from_numpy(ll.lon_edges_rad.copy()).to(DEV)
    counts = torch.zeros(40, dtype=torch.int32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    for field, bad in (('N', 0), ('N', 1 << 20), ('n_lat', 0), ('n_lon', 1), ('dust', -1.)):
        e = nat.OverlapDesc.from_buffer_copy(d)
        setattr(e, field, bad)
        assert lib.dlwpcs_overlap_count(ctypes.byref(e), sl.data_ptr(), lo.data_ptr(), counts.data_ptr(), s) == -1
    assert lib.dlwpcs_overlap_count(ctypes.byref(d), None, lo.data_ptr(), counts.data_ptr(), s) == -1
    nat.check(lib.dlwpcs_overlap_count(ctypes.byref(d), sl.data_ptr(), lo.data_ptr(), counts.data_ptr(), s), 'count')
    assert int(counts.sum()) == oc.CASES['B'][2]
    # a row_ptr that claims more than the buffers hold: nothing at or beyond nnz is written
    nnz = 100
    row_ptr = torch.zeros(41, dtype=torch.int64, device=DEV)
    torch.cumsum(counts, 0, dtype=torch.int64, out=row_ptr[1:])
    col = torch.full((nnz + 64,), -7, dtype=torch.int32, device=DEV)
    area = torch.full((nnz + 64,), -7., dtype=torch.float64, device=DEV)
    nat.check(lib.dlwpcs_overlap_fill(ctypes.byref(d), sl.data_ptr(), lo.data_ptr(), row_ptr.data_ptr(), col.data_ptr(),
                                      area.data_ptr(), nnz, s), 'fill')
    torch.cuda.synchronize()
    h_ptr, h_col, h_area = oc.host_overlap('B')
    assert (col[nnz:] == -7).all() and (area[nnz:] == -7.).all()
    assert np.array_equal(col[:nnz].cpu().numpy(), h_col[:nnz])


def _bar(m, x):
    """tests/test_gpu_remap.py's: 4e-6 * max|x| * max_row sum|S|"""
    r = np.repeat(np.arange(m.n_b), np.diff(m.row_ptr.astype(np.int64)))
    return 4e-6 * float(np.abs(x).max()) * float(np.bincount(r, np.abs(m.val64), minlength=1).max())


@pytest.mark.parametrize('name', ['A', 'C'])
def test_generate_maps_on_the_device(name):
    from DLWP.remap import CubeSphereRemap, conservative_maps
    cube, ll = oc.grids(name)
    r = CubeSphereRemap(verbose=False)
    fwd, inv = r.generate_maps(grid=cube, latlon=ll, device=DEV)
    h_fwd, h_inv = conservative_maps(cube, ll)
    for m, h in ((fwd, h_fwd), (inv, h_inv)):
        assert np.array_equal(m.row_ptr, h.row_ptr) and np.array_equal(m.col, h.col)
        assert np.abs(m.val64 - h.val64).max() <= 1e-12
    g = torch.Generator(device=DEV).manual_seed(4)
    x = torch.randn((3,) + ll.shape + (2,), generator=g, device=DEV)
    y = r.remap_array(x, axes=(1, 2))
    want = fwd.apply_host(x.cpu().numpy().astype(np.float64), (1, 2))
    assert tuple(y.shape) == (3,) + cube.shape + (2,)
    assert np.abs(y.cpu().numpy() - want).max() <= _bar(fwd, x.cpu().numpy())
    z = r.inverse_remap_array(y, axes=(1, 2, 3))
    want = inv.apply_host(y.cpu().numpy().astype(np.float64), (1, 2, 3))
    assert tuple(z.shape) == tuple(x.shape)
    assert np.abs(z.cpu().numpy() - want).max() <= _bar(inv, y.cpu().numpy())
    const = torch.full(ll.shape, 3.25, device=DEV)
    back = r.inverse_remap_array(r.remap_array(const))
    assert np.abs(back.cpu().numpy() - 3.25).max() <= 2 * _bar(fwd, np.array([3.25]))


def test_geography_on_the_device():
    from DLWP.remap import CubeSphereRemap
    cube, ll = oc.grids('A')
    r = CubeSphereRemap(verbose=False)
    fwd, _ = r.generate_maps(6, 12, 4, device=DEV)
    oc.check_geography(lambda x: fwd.apply_host(x, (0, 1)))                       # the device-made map, fp64 weights
    # and applied where it was made: fp32 weights and sums, within the remapping tests' bound of an exact 0 or 1
    _, llg = oc.grids('A')
    north = torch.from_numpy(np.broadcast_to((llg.lat > 0)[:, None], llg.shape).astype(np.float32)).to(DEV)
    east = torch.from_numpy(np.broadcast_to(((llg.lon >= 0) & (llg.lon < 180))[None, :], llg.shape).astype(np.float32)).to(DEV)
    bar = _bar(fwd, np.ones(1))
    y = r.remap_array(north).cpu().numpy()
    assert np.abs(y[5] - 1.).max() <= bar and np.abs(y[4]).max() <= bar and np.abs(y[:4, 2:] - 1.).max() <= bar
    y = r.remap_array(east).cpu().numpy()
    assert np.abs(y[1] - 1.).max() <= bar and np.abs(y[3]).max() <= bar
