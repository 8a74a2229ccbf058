"""
Synthetic offline maps for the remapping tests and tools/bench_remap.py.

These are NOT TempestRemap maps.  They have the structure of a first-order conservative map between an equiangular gnomonic
cubed sphere (any orientation) and a regular lat-lon grid: every destination cell is sampled at s x s sub-points evenly spaced
in its own coordinates, each sub-point is located in the source grid, and the weight of a source cell is the fraction of the
sub-points that fall in it.  Rows sum to 1, their lengths (a few entries) and locality are those of such a map.  With s a
power of two the weights are exact in fp32.

Cube cells are numbered face-major, (face, height, width) -> (f * N + i) * N + j; faces 0-3 are equatorial (centred on
longitudes 0, 90, 180, 270), 4 is the north and 5 the south pole.  Lat-lon cells are numbered lat-major, (lat, lon).
"""
import numpy as np


def _frames(rotation=None):
    """(6, 3, 3): per face the centre, the width direction and the height direction"""
    fr = []
    for k in range(4):
        phi = k * np.pi / 2
        fr.append([(np.cos(phi), np.sin(phi), 0.), (-np.sin(phi), np.cos(phi), 0.), (0., 0., 1.)])
    fr.append([(0., 0., 1.), (0., 1., 0.), (-1., 0., 0.)])
    fr.append([(0., 0., -1.), (0., 1., 0.), (1., 0., 0.)])
    fr = np.array(fr, dtype=np.float64)
    if rotation is not None:
        fr = fr @ np.asarray(rotation, dtype=np.float64).T
    return fr


def rotation(yaw_deg=0., pitch_deg=0., roll_deg=0.):
    """rotation matrix of the cube: about z (yaw), then y (pitch), then x (roll)"""
    a, b, c = np.deg2rad([yaw_deg, pitch_deg, roll_deg])
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    rx = np.array([[1, 0, 0], [0, np.cos(c), -np.sin(c)], [0, np.sin(c), np.cos(c)]])
    return rx @ ry @ rz


def _cube_points(N, fr, fi, i, j):
    """unit vectors of the cube points at fractional cell coordinates (i: height, j: width) on faces fi"""
    h = np.pi / (2 * N)
    ta, tb = np.tan(-np.pi / 4 + j * h), np.tan(-np.pi / 4 + i * h)
    p = fr[fi, 0] + ta[:, None] * fr[fi, 1] + tb[:, None] * fr[fi, 2]
    return p / np.linalg.norm(p, axis=1, keepdims=True)


def _locate_cube(N, fr, p):
    d = p @ fr[:, 0].T                                    # (n, 6): the containing face has the largest dot product
    f = np.argmax(d, axis=1)
    dc = d[np.arange(p.shape[0]), f]
    u = np.einsum('nk,nk->n', p, fr[f, 1]) / dc
    v = np.einsum('nk,nk->n', p, fr[f, 2]) / dc
    h = np.pi / (2 * N)
    j = np.clip(np.floor((np.arctan(u) + np.pi / 4) / h), 0, N - 1).astype(np.int64)
    i = np.clip(np.floor((np.arctan(v) + np.pi / 4) / h), 0, N - 1).astype(np.int64)
    return (f * N + i) * N + j


def _latlon(lat, lon):
    la, lo = np.deg2rad(lat), np.deg2rad(lon)
    return np.stack([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)], axis=1)


class LatLon(object):
    """n_lat x n_lon cells spanning [lat_begin, lat_end] x [lon_begin, lon_begin + 360)"""

    def __init__(self, n_lat, n_lon, descending=False, lon_begin=0.):
        self.n_lat, self.n_lon = int(n_lat), int(n_lon)
        self.lat0, self.dlat = (90., -180. / n_lat) if descending else (-90., 180. / n_lat)
        self.lon0, self.dlon = float(lon_begin), 360. / n_lon
        self.lat = self.lat0 + (np.arange(n_lat) + 0.5) * self.dlat
        self.lon = self.lon0 + (np.arange(n_lon) + 0.5) * self.dlon

    def centres(self):
        la, lo = np.meshgrid(self.lat, self.lon, indexing='ij')
        return la.ravel(), lo.ravel()

    def locate(self, p):
        lat = np.rad2deg(np.arcsin(np.clip(p[:, 2], -1, 1)))
        lon = np.rad2deg(np.arctan2(p[:, 1], p[:, 0]))
        i = np.clip(np.floor((lat - self.lat0) / self.dlat), 0, self.n_lat - 1).astype(np.int64)
        j = np.clip(np.floor(np.mod(lon - self.lon0, 360.) / self.dlon), 0, self.n_lon - 1).astype(np.int64)
        return i * self.n_lon + j

    def subpoints(self, s):
        """(cell index, unit vector) of the s x s sub-points of every cell"""
        off = (np.arange(s) + 0.5) / s
        ci, cj, a, b = np.meshgrid(np.arange(self.n_lat), np.arange(self.n_lon), off, off, indexing='ij')
        lat = self.lat0 + (ci + a).ravel() * self.dlat
        lon = self.lon0 + (cj + b).ravel() * self.dlon
        return (ci * self.n_lon + cj).ravel(), _latlon(lat, lon)


class Cube(object):
    """equiangular gnomonic cubed sphere of N x N cells per face, turned by `rotation` (3 x 3) if given"""

    def __init__(self, N, rotation=None):
        self.N = int(N)
        self.fr = _frames(rotation)

    def centres(self):
        N = self.N
        f, i, j = np.meshgrid(np.arange(6), np.arange(N), np.arange(N), indexing='ij')
        p = _cube_points(N, self.fr, f.ravel(), i.ravel() + 0.5, j.ravel() + 0.5)
        return np.rad2deg(np.arcsin(np.clip(p[:, 2], -1, 1))), np.mod(np.rad2deg(np.arctan2(p[:, 1], p[:, 0])), 360.)

    def locate(self, p):
        return _locate_cube(self.N, self.fr, p)

    def subpoints(self, s):
        N = self.N
        off = (np.arange(s) + 0.5) / s
        f, i, j, a, b = np.meshgrid(np.arange(6), np.arange(N), np.arange(N), off, off, indexing='ij')
        return ((f * N + i) * N + j).ravel(), _cube_points(N, self.fr, f.ravel(), (i + a).ravel(), (j + b).ravel())


def _dims(g):
    return np.array([6 * g.N * g.N] if isinstance(g, Cube) else [g.n_lon, g.n_lat], dtype=np.int32)


def map_arrays(src, dst, s=4):
    """the SCRIP-layout arrays (row / col 1-based, S, grid dims, yc / xc in degrees) of the map src -> dst"""
    rows, pts = dst.subpoints(s)
    cols = src.locate(pts)
    n_a = 6 * src.N ** 2 if isinstance(src, Cube) else src.n_lat * src.n_lon
    n_b = 6 * dst.N ** 2 if isinstance(dst, Cube) else dst.n_lat * dst.n_lon
    key, cnt = np.unique(rows * n_a + cols, return_counts=True)
    yc_a, xc_a = src.centres()
    yc_b, xc_b = dst.centres()
    return dict(row=(key // n_a + 1).astype(np.int32), col=(key % n_a + 1).astype(np.int32), S=cnt / float(s * s),
                n_a=n_a, n_b=n_b, src_grid_dims=_dims(src), dst_grid_dims=_dims(dst), yc_a=yc_a, xc_a=xc_a, yc_b=yc_b,
                xc_b=xc_b)


def make_map(src, dst, s=4):
    from DLWP.remap import OfflineMap
    return OfflineMap(**map_arrays(src, dst, s))


def cube_to_latlon(N, n_lat, n_lon, s=4, rotation=None, descending=False):
    return make_map(Cube(N, rotation), LatLon(n_lat, n_lon, descending), s)


def latlon_to_cube(n_lat, n_lon, N, s=4, rotation=None, descending=False):
    return make_map(LatLon(n_lat, n_lon, descending), Cube(N, rotation), s)


def random_map(rng, n_a, n_b, nnz, empty_rows=0, duplicates=0, shuffle=True):
    """an OfflineMap of random entries: `empty_rows` rows without entries, `duplicates` repeated (row, col) pairs, entries
    in random order (unsorted rows)"""
    from DLWP.remap import OfflineMap
    live = rng.permutation(n_b)[:max(n_b - empty_rows, 1)]
    row = rng.choice(live, nnz)
    col = rng.integers(0, n_a, nnz)
    S = rng.standard_normal(nnz)
    if duplicates:
        k = rng.integers(0, nnz, duplicates)
        row, col, S = np.r_[row, row[k]], np.r_[col, col[k]], np.r_[S, rng.standard_normal(duplicates)]
    if not shuffle:
        o = np.argsort(row, kind='stable')
        row, col, S = row[o], col[o], S[o]
    return OfflineMap(row + 1, col + 1, S, n_a, n_b)


def dense(m):
    """the map as a dense fp64 (n_b, n_a) matrix"""
    D = np.zeros((m.n_b, m.n_a))
    r = np.repeat(np.arange(m.n_b), np.diff(m.row_ptr.astype(np.int64)))
    np.add.at(D, (r, m.col.astype(np.int64)), m.val64)
    return D
