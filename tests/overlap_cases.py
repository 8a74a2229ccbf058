"""
The grids shared by the map-generation tests (tests/test_overlap.py, tests/test_gpu_overlap.py) with the entry counts their
overlap matrices must have after dust removal, and the host twin's result for each, computed once.
"""
import functools

import numpy as np

# name: (N, how the lat-lon grid is made, entries)
CASES = {
    'A': (4, ('cells', 6, 12, False, 0.), 264),
    'B': (3, ('cells', 5, 8, False, -7.), 188),
    'C': (4, ('centres', 7, 12, -15.), 304),
    'D': (5, ('cells', 9, 16, False, 0.), 560),
    'D_inverse': (5, ('cells', 9, 16, True, 0.), 560),
    'E': (8, ('cells', 12, 24, False, 0.), 1168),
    'F': (6, ('cells', 10, 20, False, 3.), 784),
}


def latlon_grid(spec):
    from DLWP.remap import LatLonGrid
    if spec[0] == 'cells':
        return LatLonGrid.cells(spec[1], spec[2], inverse_lat=spec[3], lon_begin=spec[4])
    n_lat, n_lon, lon_begin = spec[1:]
    d = 360. / n_lon
    return LatLonGrid.from_centres(np.linspace(-90., 90., n_lat), lon_begin + d * (np.arange(n_lon) + 0.5))


@functools.lru_cache(maxsize=None)
def grids(name):
    from DLWP.remap import CubeSphereGrid
    N, spec, _ = CASES[name]
    return CubeSphereGrid(N), latlon_grid(spec)


@functools.lru_cache(maxsize=None)
def host_overlap(name):
    """(row_ptr, col, area) of the host twin; treat as read-only"""
    from DLWP.remap import overlap_areas
    cube, ll = grids(name)
    out = overlap_areas(cube, ll)
    for a in out:
        a.setflags(write=False)
    return out


def rows_of(row_ptr):
    return np.repeat(np.arange(row_ptr.size - 1), np.diff(row_ptr))


def marginal_residuals(cube, ll, row_ptr, col, area):
    """largest relative residual of the row sums against the lat-lon cell areas and of the column sums against the cube's"""
    r = rows_of(row_ptr)
    ar, ac = ll.area.ravel(), cube.area.ravel()
    return (float(np.abs(np.bincount(r, area, ll.n_cells) / ar - 1.).max()),
            float(np.abs(np.bincount(col, area, cube.n_cells) / ac - 1.).max()))


def check_geography(remap_fn):
    """on A (edges on the hemispheres): remap_fn takes a (6, 12) lat-lon field to (6, 4, 4)"""
    _, ll = grids('A')
    north = np.broadcast_to((ll.lat > 0)[:, None], ll.shape).astype(np.float64)
    y = remap_fn(north)
    assert np.abs(y[5] - 1.).max() <= 1e-12 and np.abs(y[4]).max() <= 1e-12
    assert np.abs(y[:4, 2:] - 1.).max() <= 1e-12 and np.abs(y[:4, :2]).max() <= 1e-12
    east = np.broadcast_to(((ll.lon >= 0) & (ll.lon < 180))[None, :], ll.shape).astype(np.float64)
    y = remap_fn(east)
    assert np.abs(y[1] - 1.).max() <= 1e-12 and np.abs(y[3]).max() <= 1e-12
