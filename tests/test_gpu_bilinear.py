"""
Bilinear sampling weights on the device (dlwpcs_cube_bilinear, csrc/bilinear.hip): the kernel against the numpy twin on points
whose dual face is known by construction, the property checks on points that sit on the boundaries of dual faces, the ABI's
refusals and its writes, CubeSphereRemap.generate_sampling_map with device tensors sampled by the map it made, and one larger run.
The cubes are the smallest at which every branch runs: N = 1 (triangles only), 2 (no interior quadrilateral away from a border),
3, 5, 8 and a mirrored rotated 5.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bilinear_cases as bc   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAMES = sorted(bc.CUBES)


def _device_weights(cb, lat, lon):
    from DLWP.remap import point_weights
    col, w = point_weights(cb, lat, lon, device=DEV)
    torch.cuda.synchronize()
    assert col.is_cuda and w.is_cuda and col.dtype == torch.int32 and w.dtype == torch.float64
    return col, w


@pytest.mark.parametrize('name', NAMES)
def test_kernel_against_the_host_twin(name):
    """|w_dev - w_host| <= 1e-11 is derived: a position error of about 1e-16 over a cell width of at least pi / 2048, with a
    margin of 100."""
    cb = bc.cube(name)
    lat, lon = bc.interior(name)[:2]
    first = _device_weights(cb, lat, lon)
    col, w = (t.cpu().numpy() for t in first)
    h_col, h_w = bc.host_weights(name, 'interior')
    assert col.shape == h_col.shape and np.array_equal(col, h_col)
    diff = float(np.abs(w - h_w).max())
    print('%s: %d points, device - host %.3g' % (name, lat.size, diff))
    assert diff <= 1e-11
    second = _device_weights(cb, lat, lon)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


@pytest.mark.parametrize('name', NAMES)
def test_boundary_points_have_the_properties(name):
    """on a side of a dual face either neighbour is a right answer: no comparison of cells, the sampled values must agree"""
    cb = bc.cube(name)
    lat, lon, own = bc.boundary(name)
    col, w = (t.cpu().numpy() for t in _device_weights(cb, lat, lon))
    res = bc.check_properties(cb, lat, lon, col, w, own)
    h_col, h_w = bc.host_weights(name, 'boundary')
    diff = float(np.abs(bc.sample(cb, col, w) - bc.sample(cb, h_col, h_w)).max())
    print('%s: %d points, residuals %.3g (sum) %.3g (direction), sampled values device - host %.3g' % ((name, lat.size) + res + (diff,)))
    assert diff <= 1e-11


def _desc(cb, n):
    from DLWP import _native as nat
    from DLWP.remap.bilinear import cube_edges
    d = nat.CubeBilinearDesc()
    d.N, d.n_points = cb.N, n
    fr = np.ascontiguousarray(cb.frames)
    ctypes.memmove(ctypes.addressof(d.frames), fr.ctypes.data, fr.nbytes)
    ed = np.ascontiguousarray(cube_edges())
    ctypes.memmove(ctypes.addressof(d.edge), ed.ctypes.data, ed.nbytes)
    return d


def test_abi_refuses_bad_descriptors_and_writes_stay_inside():
    from DLWP import _native as nat
    cb = bc.cube('N3')
    lat, lon = bc.boundary('N3')[:2]
    n, guard = lat.size, 64
    lib = nat.lib()
    s = torch.cuda.current_stream().cuda_stream
    la, lo = torch.from_numpy(lat.copy()).to(DEV), torch.from_numpy(lon.copy()).to(DEV)
    col = torch.full((4 * n + 2 * guard,), -7, dtype=torch.int32, device=DEV)
    w = torch.full((4 * n + 2 * guard,), -7., dtype=torch.float64, device=DEV)
    args = (la.data_ptr(), lo.data_ptr(), col[guard:].data_ptr(), w[guard:].data_ptr(), s)
    d = _desc(cb, n)

    def bad(change):
        e = nat.CubeBilinearDesc.from_buffer_copy(d)
        change(e)
        return lib.dlwpcs_cube_bilinear(ctypes.byref(e), *args)

    def set_n(v):
        return lambda e: setattr(e, 'N', v)

    def skew(e):
        e.frames[2][1][0] += 1e-6

    def edge(f, side, k, v):
        def change(e):
            e.edge[f][side][k] = v
        return change

    for change in (set_n(0), set_n(-3), lambda e: setattr(e, 'n_points', -1), skew, edge(0, 0, 0, 6), edge(5, 3, 0, -1),
                   edge(1, 2, 1, 4), edge(4, 1, 2, 2)):
        assert bad(change) == -1
    assert b'cube_bilinear' in lib.dlwpcs_last_error()
    assert lib.dlwpcs_cube_bilinear(ctypes.byref(d), None, lo.data_ptr(), col.data_ptr(), w.data_ptr(), s) == -1
    torch.cuda.synchronize()
    assert (col == -7).all() and (w == -7.).all()                   # a refused call launches nothing
    # no points: no launch, whatever the pointers are
    assert lib.dlwpcs_cube_bilinear(ctypes.byref(_desc(cb, 0)), None, None, None, None, s) == 0
    nat.check(lib.dlwpcs_cube_bilinear(ctypes.byref(d), *args), 'dlwpcs_cube_bilinear')
    torch.cuda.synchronize()
    assert (col[:guard] == -7).all() and (col[guard + 4 * n:] == -7).all()
    assert (w[:guard] == -7.).all() and (w[guard + 4 * n:] == -7.).all()
    h_col, h_w = bc.host_weights('N3', 'boundary')
    got_c, got_w = col[guard:guard + 4 * n].cpu().numpy().reshape(n, 4), w[guard:guard + 4 * n].cpu().numpy().reshape(n, 4)
    bc.check_properties(cb, lat, lon, got_c, got_w)
    assert np.abs(bc.sample(cb, got_c, got_w) - bc.sample(cb, h_col, h_w)).max() <= 1e-11


def test_a_point_that_cannot_be_placed_gets_cell_0_and_nan():
    """the Python layer never sends one; the kernel still writes only cells of the cube"""
    from DLWP import _native as nat
    cb = bc.cube('N2')
    la = torch.tensor([10., float('nan'), 20., float('inf'), -30.], dtype=torch.float64, device=DEV)
    lo = torch.tensor([5., 5., float('nan'), 7., 1e300], dtype=torch.float64, device=DEV)
    col = torch.full((5, 4), -7, dtype=torch.int32, device=DEV)
    w = torch.full((5, 4), -7., dtype=torch.float64, device=DEV)
    nat.check(nat.lib().dlwpcs_cube_bilinear(ctypes.byref(_desc(cb, 5)), la.data_ptr(), lo.data_ptr(), col.data_ptr(), w.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream), 'dlwpcs_cube_bilinear')
    torch.cuda.synchronize()
    col, w = col.cpu().numpy(), w.cpu().numpy()
    assert col.min() >= 0 and col.max() < cb.n_cells
    assert (col[1:4] == 0).all() and np.isnan(w[1:4]).all()
    assert np.all(w[[0, 4]] >= 0) and np.abs(w[[0, 4]].sum(axis=1) - 1.).max() <= 1e-14


def test_python_layer_checks_before_the_launch_and_keeps_device_inputs():
    from DLWP.remap import point_weights
    cb = bc.cube('N3')
    for lat, lon in (([91.], [0.]), ([np.nan], [0.]), ([0.], [np.inf])):
        with pytest.raises(ValueError):
            point_weights(cb, lat, lon, device=DEV)
        with pytest.raises(ValueError):
            point_weights(cb, torch.tensor(lat, dtype=torch.float64, device=DEV), torch.tensor(lon, dtype=torch.float64, device=DEV),
                          device=DEV)
    lat, lon = bc.interior('N3')[:2]
    col, w = point_weights(cb, torch.from_numpy(lat.copy()).to(DEV), torch.from_numpy(lon.copy()).to(DEV), device=DEV)
    h_col, h_w = bc.host_weights('N3', 'interior')
    assert col.is_cuda and w.is_cuda
    assert np.array_equal(col.cpu().numpy(), h_col) and np.abs(w.cpu().numpy() - h_w).max() <= 1e-11
    col, w = point_weights(cb, np.zeros((0,)), np.zeros((0,)), device=DEV)
    assert tuple(col.shape) == (0, 4) and tuple(w.shape) == (0, 4)


def test_sampling_on_the_device_end_to_end():
    """generate_sampling_map on the device, then sample_array of fp32 and bf16 device tensors against apply_host of the same map:
    fp32 weights and sums of four terms, relative 1e-6 of max|x| (4 * 2^-24 * 3 rounded operations is 7e-7); the bf16 input is
    compared after its own rounding, so the same bound holds."""
    from DLWP.model.extensions import Forecast
    from DLWP.remap import CubeSphereRemap, LatLonGrid, bilinear_map
    cb = bc.cube('N8')
    rng = np.random.default_rng(8)
    lat, lon = rng.uniform(-90, 90, 301), rng.uniform(-360, 720, 301)
    r = CubeSphereRemap(verbose=False)
    m = r.generate_sampling_map(lat, lon, grid=cb, device=DEV)
    h = bilinear_map(cb, lat, lon)
    assert m.dst_kind == 'cells' and m.dst_shape == (301,)
    assert np.array_equal(m.col, h.col) and np.abs(m.val64 - h.val64).max() <= 1e-11
    g = torch.Generator(device=DEV).manual_seed(4)
    x = torch.randn((5, 3) + cb.shape, generator=g, device=DEV)
    for xt in (x, x.to(torch.bfloat16)):
        y = r.sample_array(xt)
        xin = xt.to(torch.float32).cpu().numpy().astype(np.float64)
        want = m.apply_host(xin, (2, 3, 4))
        assert y.is_cuda and y.dtype == torch.float32 and tuple(y.shape) == (5, 3, 301)
        assert np.abs(y.cpu().numpy() - want).max() <= 1e-6 * np.abs(xin).max()
    fc = Forecast(x, ('f_hour', 'time', 'x0', 'x1', 'x2'), {'f_hour': np.arange(5), 'time': np.arange(3)})
    out = r.sample_forecast(fc)
    assert out.values.is_cuda and out.dims == ('f_hour', 'time', 'point') and tuple(out.values.shape) == (5, 3, 301)
    assert torch.equal(out.values, r.sample_array(x))
    ll = LatLonGrid.cells(24, 48)
    mg = r.generate_sampling_map(latlon=ll, grid=cb, device=DEV)
    hg = bilinear_map(cb, latlon=ll)
    assert mg.dst_kind == 'latlon' and np.array_equal(mg.col, hg.col) and np.abs(mg.val64 - hg.val64).max() <= 1e-11
    out = r.sample_forecast(fc)
    assert out.values.is_cuda and out.dims == ('f_hour', 'time', 'lat', 'lon') and tuple(out.values.shape) == (5, 3, 24, 48)
    want = hg.apply_host(x.cpu().numpy().astype(np.float64), (2, 3, 4))
    assert np.abs(out.values.cpu().numpy() - want).max() <= 1e-6 * float(x.abs().max())


def test_identities_c48_pole_centred():
    """the centres of 181 x 360 (rows on both poles) on C48: property checks only"""
    from DLWP.remap import CubeSphereGrid
    cb = CubeSphereGrid(48)
    lat, lon = (a.ravel() for a in np.meshgrid(np.linspace(-90., 90., 181), np.arange(360.), indexing='ij'))
    col, w = (t.cpu().numpy() for t in _device_weights(cb, lat, lon))
    res = bc.check_properties(cb, lat, lon, col, w)
    print('C48 at 181 x 360 centres: residuals %.3g (sum), %.3g (direction)' % res)
