"""
CPU tests of DLWP.remap: the netCDF classic / 64-bit-offset reader against fixtures written by an independent writer
(tests/golden/gen_golden_remap.py, scipy.io.netcdf_file), load-time validation, grid orientation, the fp64 host path against a
dense matrix product, labelled forecasts and the file-to-file methods.
"""
import os

import numpy as np
import pytest

import remap_maps as rm
from DLWP.model.extensions import Forecast
from DLWP.remap import CubeSphereRemap, OfflineMap, read_offline_map
from DLWP.remap.netcdf_classic import NetCDFClassic
from DLWP.verify import forecast_error

FILES = {'classic': 'g14_map_classic.nc', '64bit': 'g14_map_64bit.nc'}
VARS = ('row', 'col', 'S', 'src_grid_dims', 'dst_grid_dims', 'yc_a', 'xc_a', 'yc_b', 'xc_b', 'frac_b')


@pytest.fixture(scope='module')
def expected(golden_dir):
    return np.load(os.path.join(golden_dir, 'g14_remap.npz'))


@pytest.mark.parametrize('tag', sorted(FILES))
def test_reader_reproduces_the_written_arrays(golden_dir, expected, tag):
    nc = NetCDFClassic(os.path.join(golden_dir, FILES[tag]))
    assert nc.version == (1 if tag == 'classic' else 2)
    assert nc.dims['n_a'] == int(expected[tag + '/n_a']) and nc.dims['n_b'] == int(expected[tag + '/n_b'])
    assert nc.dims['n_s'] == expected[tag + '/row'].size
    for v in VARS:
        got, want = nc.read(v), expected['%s/%s' % (tag, v)]
        assert got.dtype == want.dtype.newbyteorder('=') and np.array_equal(got, want), v
    assert nc.variables['yc_a'][2]['units'] == 'degrees'


def test_reader_reads_record_variables(golden_dir, expected):
    nc = NetCDFClassic(os.path.join(golden_dir, FILES['64bit']))
    assert nc.dims['rec'] == 4
    for v in ('rec_a', 'rec_b'):
        assert np.array_equal(nc.read(v), expected['64bit/' + v])


@pytest.mark.parametrize('tag', sorted(FILES))
def test_read_offline_map_builds_the_csr(golden_dir, expected, tag):
    m = read_offline_map(os.path.join(golden_dir, FILES[tag]))
    e = {v: expected['%s/%s' % (tag, v)] for v in VARS}
    ref = OfflineMap(e['row'], e['col'], e['S'], int(expected[tag + '/n_a']), int(expected[tag + '/n_b']),
                     e['src_grid_dims'], e['dst_grid_dims'], e['yc_a'], e['xc_a'], e['yc_b'], e['xc_b'])
    for a in ('row_ptr', 'col', 'val', 'val64'):
        assert np.array_equal(getattr(m, a), getattr(ref, a)), a
    assert m.row_ptr.dtype == np.int32 and m.col.dtype == np.int32 and m.val.dtype == np.float32
    assert np.array_equal(m.frac_b, e['frac_b'])
    cube, ll = (6, 4, 4), (5, 8)
    assert (m.src_shape, m.dst_shape) == ((cube, ll) if tag == 'classic' else (ll, cube))
    lat = (m.lat_b if tag == 'classic' else m.lat_a)
    assert np.allclose(lat, rm.LatLon(5, 8).lat) and np.allclose(np.abs(rm.dense(m).sum(1)), 1.)


def test_netcdf4_file_is_refused_with_the_conversion(golden_dir):
    with pytest.raises(ValueError, match='netCDF-4') as e:
        read_offline_map(os.path.join(golden_dir, 'h5_weights_tiny.h5'))
    assert 'nccopy -k 64-bit-offset' in str(e.value) and 'to_netcdf4=False' in str(e.value)


def test_truncated_file_raises(golden_dir, tmp_path):
    raw = open(os.path.join(golden_dir, FILES['classic']), 'rb').read()
    for cut in (len(raw) - 100, 200, 30):
        p = tmp_path / ('cut%d.nc' % cut)
        p.write_bytes(raw[:cut])
        with pytest.raises(ValueError, match='truncated'):
            read_offline_map(str(p))


def test_missing_file_and_not_netcdf(tmp_path):
    with pytest.raises(FileNotFoundError):
        read_offline_map(str(tmp_path / 'nope.nc'))
    p = tmp_path / 'text.nc'
    p.write_bytes(b'hello world, not a netCDF file')
    with pytest.raises(ValueError, match='not a netCDF'):
        read_offline_map(str(p))


def _patched(golden_dir, tmp_path, name, edit):
    """a copy of the classic fixture with its bytes edited"""
    raw = bytearray(open(os.path.join(golden_dir, FILES['classic']), 'rb').read())
    edit(raw)
    p = tmp_path / name
    p.write_bytes(bytes(raw))
    return str(p)


def test_load_validation_errors(tmp_path):
    row, col, S = np.array([1, 2, 3]), np.array([1, 1, 2]), np.array([.5, .5, 1.])
    with pytest.raises(ValueError, match='row indices'):
        OfflineMap(row, col, S, 2, 2)
    with pytest.raises(ValueError, match='row indices'):
        OfflineMap(row - 1, col, S, 2, 3)
    with pytest.raises(ValueError, match='col indices'):
        OfflineMap(row, col + 1, S, 2, 3)
    with pytest.raises(ValueError, match='different lengths'):
        OfflineMap(row, col[:2], S, 2, 3)
    with pytest.raises(ValueError, match='non-finite'):
        OfflineMap(row, col, np.array([.5, np.nan, 1.]), 2, 3)
    with pytest.raises(ValueError, match='grid_dims'):
        OfflineMap(row, col, S, 2, 3, dst_grid_dims=[2, 2])


def test_file_validation_errors(golden_dir, tmp_path):
    def rename_s(raw):                  # the variable name 'S' (length 1, padded to 4) becomes 'Q'
        k = raw.index(b'\x00\x00\x00\x01S\x00\x00\x00')
        raw[k + 4] = ord('Q')

    with pytest.raises(ValueError, match="variable.*S.*missing"):
        read_offline_map(_patched(golden_dir, tmp_path, 'no_s.nc', rename_s))
    begin = NetCDFClassic(os.path.join(golden_dir, FILES['classic']))._vars['row'][4]

    def big_row(raw):
        raw[begin:begin + 4] = np.array([10 ** 6], '>i4').tobytes()

    with pytest.raises(ValueError, match='row indices'):
        read_offline_map(_patched(golden_dir, tmp_path, 'big_row.nc', big_row))


def test_empty_rows_duplicates_and_unsorted_entries_in_the_csr():
    m = OfflineMap([3, 1, 3, 3, 1], [2, 1, 2, 1, 2], [1., 2., 3., 4., 5.], 2, 4)
    assert list(m.row_ptr) == [0, 2, 2, 5, 5]
    assert list(m.col) == [0, 1, 1, 1, 0] and list(m.val64) == [2., 5., 1., 3., 4.]


def _ll_arrays(n_lat, n_lon, lon_major):
    ll = rm.LatLon(n_lat, n_lon)
    la, lo = np.meshgrid(ll.lat, ll.lon, indexing='xy' if lon_major else 'ij')
    return la.ravel(), lo.ravel()


def test_lon_major_destination_is_transposed():
    a = rm.map_arrays(rm.Cube(3), rm.LatLon(4, 6), s=2)
    ref = OfflineMap(**a)
    # the same map with the destination stored lon-major (latitude fastest) and dims in that order
    i_lat, i_lon = np.divmod(a['row'] - 1, 6)
    b = dict(a, row=(i_lon * 4 + i_lat + 1).astype(np.int32), dst_grid_dims=np.array([4, 6], np.int32))
    b['yc_b'], b['xc_b'] = _ll_arrays(4, 6, lon_major=True)
    m = OfflineMap(**b)
    assert m.dst_shape == (4, 6) and np.allclose(m.lat_b, ref.lat_b) and np.allclose(m.lon_b, ref.lon_b)
    x = np.random.default_rng(0).standard_normal((2, 6, 3, 3))
    assert np.array_equal(m.apply_host(x, (1, 2, 3)), ref.apply_host(x, (1, 2, 3)))
    assert np.allclose(m.yc_b, ref.yc_b)


def test_lon_major_source_is_transposed():
    a = rm.map_arrays(rm.LatLon(4, 6), rm.Cube(3), s=2)
    ref = OfflineMap(**a)
    i_lat, i_lon = np.divmod(a['col'] - 1, 6)
    b = dict(a, col=(i_lon * 4 + i_lat + 1).astype(np.int32), src_grid_dims=np.array([4, 6], np.int32))
    b['yc_a'], b['xc_a'] = _ll_arrays(4, 6, lon_major=True)
    m = OfflineMap(**b)
    x = np.random.default_rng(1).standard_normal((4, 6, 2))
    assert m.src_shape == (4, 6) and np.array_equal(m.apply_host(x, (0, 1)), ref.apply_host(x, (0, 1)))


def test_inconsistent_latitudes_raise():
    a = rm.map_arrays(rm.Cube(3), rm.LatLon(4, 6), s=2)
    yc = a['yc_b'].copy()
    yc[7] += 1.
    with pytest.raises(ValueError, match='latitude must be constant'):
        OfflineMap(**dict(a, yc_b=yc))


@pytest.mark.parametrize('seed', range(4))
def test_host_path_equals_dense_product(seed):
    rng = np.random.default_rng(seed)
    n_a, n_b = int(rng.integers(5, 40)), int(rng.integers(5, 40))
    m = rm.random_map(rng, n_a, n_b, int(rng.integers(1, 4 * n_b)), empty_rows=3, duplicates=5)
    D = rm.dense(m)
    assert (np.diff(m.row_ptr) == 0).any()
    x = rng.standard_normal((3, n_a, 4))
    want = np.einsum('ba,pak->pbk', D, x)
    # the space axis first, in the middle and last
    assert np.abs(m.apply_host(np.moveaxis(x, 1, 0), 0) - np.moveaxis(want, 1, 0)).max() <= 1e-12
    assert np.abs(m.apply_host(x, 1) - want).max() <= 1e-12
    assert np.abs(m.apply_host(np.moveaxis(x, 1, 2), -1) - np.moveaxis(want, 1, 2)).max() <= 1e-12


def test_host_path_dtypes_and_grid_axes():
    m = rm.cube_to_latlon(4, 5, 8, s=2)
    rng = np.random.default_rng(2)
    x = rng.standard_normal((2, 6, 4, 4, 3)).astype(np.float32)
    y = m.apply_host(x, (1, 2, 3))
    assert y.dtype == np.float32 and y.shape == (2, 5, 8, 3)
    y64 = m.apply_host(x.astype(np.float64), (-4, -3, -2))
    assert y64.dtype == np.float64 and np.allclose(y, y64, atol=1e-6)
    flat = m.apply_host(x.reshape(2, 96, 3), 1)                  # one axis of n_a cells
    assert np.array_equal(flat, y)
    assert m.apply_host(np.ones((6, 4, 4), np.int32), (0, 1, 2)).dtype == np.float64
    with pytest.raises(ValueError, match='consecutive'):
        m.apply_host(x, (1, 3, 4))
    with pytest.raises(ValueError, match='shape'):
        m.apply_host(x, (2, 3, 4))


def test_cube_sphere_remap_array_methods(tmp_path):
    fw, bw = rm.latlon_to_cube(5, 8, 4, s=2), rm.cube_to_latlon(4, 5, 8, s=2)
    r = CubeSphereRemap(verbose=False)
    with pytest.raises(ValueError, match='assign_maps'):
        r.remap_array(np.zeros((5, 8)))
    r.assign_maps(fw, bw)
    x = np.random.default_rng(3).standard_normal((7, 5, 8))
    cs = r.remap_array(x)
    assert cs.shape == (7, 6, 4, 4) and np.array_equal(cs, fw.apply_host(x, (1, 2)))
    assert r.inverse_remap_array(cs).shape == (7, 5, 8)
    r2 = CubeSphereRemap(verbose=False)
    r2.assign_maps(str(tmp_path / 'missing_map.nc'))
    with pytest.raises(FileNotFoundError):
        r2.remap_array(x)


def test_cube_sphere_remap_reads_map_files(golden_dir):
    r = CubeSphereRemap(verbose=False)
    r.assign_maps(os.path.join(golden_dir, FILES['64bit']), os.path.join(golden_dir, FILES['classic']))
    x = np.ones((2, 5, 8), np.float32)
    assert np.allclose(r.remap_array(x), 1.) and np.allclose(r.inverse_remap_array(r.remap_array(x)), 1.)


@pytest.mark.parametrize('method', ['generate_offline_maps', 'generate_offline_maps_from_file', 'remap', 'inverse_remap',
                                    'convert_to_faces', 'convert_from_faces'])
def test_file_methods_are_not_implemented(method):
    with pytest.raises(NotImplementedError, match='remap_array'):
        getattr(CubeSphereRemap(verbose=False), method)('in.nc', 'out.nc')


@pytest.mark.parametrize('space', [('x0', 'x1', 'x2'), ('face', 'height', 'width')])
def test_inverse_remap_forecast_labels_and_weighted_score(space):
    rng = np.random.default_rng(4)
    m = rm.cube_to_latlon(4, 5, 8, s=2)
    r = CubeSphereRemap(verbose=False)
    r.assign_maps(inverse_map_name=m)
    dims = ('f_hour', 'time') + space + ('varlev',)
    shape = (3, 2, 6, 4, 4, 2)
    coords = {'f_hour': np.array([6., 12., 18.]), 'time': np.arange(2), 'varlev': np.array(['z500', 't850'])}
    coords.update({d: np.arange(n) for d, n in zip(space, (6, 4, 4))})
    fc = Forecast(rng.standard_normal(shape).astype(np.float32), dims, coords)
    ver = Forecast(rng.standard_normal(shape).astype(np.float32), dims, coords, name='verification')
    ver.values[2, 1] = np.nan                                       # past the end of the data
    f_ll, v_ll = r.inverse_remap_forecast(fc), r.inverse_remap_forecast(ver)
    assert f_ll.dims == ('f_hour', 'time', 'lat', 'lon', 'varlev') and f_ll.shape == (3, 2, 5, 8, 2)
    assert np.array_equal(f_ll.coords['lat'], m.lat_b) and np.array_equal(f_ll.coords['lon'], m.lon_b)
    assert np.array_equal(f_ll.coords['varlev'], coords['varlev']) and 'x0' not in f_ll.coords
    assert v_ll.lat.dims == ('lat',) and np.array_equal(np.asarray(v_ll.lat.values), m.lat_b)
    assert np.isnan(v_ll.values[2, 1]).all() and not np.isnan(v_ll.values[:2]).any()
    assert np.array_equal(f_ll.values, m.apply_host(fc.values, (2, 3, 4)))
    got = forecast_error(f_ll, v_ll, method='rmse', weighted=True)
    w = np.cos(np.deg2rad(m.lat_b))
    w = (w / w.mean())[None, None, :, None, None]
    d = w * (v_ll.values.astype(np.float64) - f_ll.values) ** 2
    want = np.sqrt(np.nanmean(d.reshape(3, -1), axis=1))
    assert got.shape == (3,) and np.allclose(got, want, rtol=1e-6)


def test_inverse_remap_forecast_needs_cube_dims():
    r = CubeSphereRemap(verbose=False)
    r.assign_maps(inverse_map_name=rm.cube_to_latlon(4, 5, 8, s=2))
    with pytest.raises(ValueError, match='x0'):
        r.inverse_remap_forecast(Forecast(np.zeros((1, 6, 4, 4)), ('f_hour', 'a', 'b', 'c'), {}))
