"""
The two grids of the remapping, in closed form (numpy, fp64): the equiangular gnomonic cubed sphere in the face layout that
CubeSpherePadding2D encodes, and a regular lat-lon grid given by its cell edges.  Both carry cell centres in degrees and cell
areas in steradians; DLWP.remap.overlap computes the areas of their cells' intersections from the same descriptions.
"""
import numpy as np

_PROCRUSTES_TOL = 1e-5           # largest distance (unit sphere) between given centres and the fitted grid's


def default_frames():
    """(6, 3, 3): per face the centre e0, the width direction eu and the height direction ev.  Faces 0-3 are centred on the
    equator at longitudes 0, 90, 180, 270; face 4 is the south and face 5 the north pole (the padding layer's layout)."""
    fr = np.zeros((6, 3, 3))
    for f, (c, s) in enumerate(((1., 0.), (0., 1.), (-1., 0.), (0., -1.))):       # cos / sin of f * 90 degrees, exactly
        fr[f] = [(c, s, 0.), (-s, c, 0.), (0., 0., 1.)]
    fr[4] = [(0., 0., -1.), (0., 1., 0.), (1., 0., 0.)]
    fr[5] = [(0., 0., 1.), (0., 1., 0.), (-1., 0., 0.)]
    return fr


def line_tangents(N):
    """(N + 1,): tan(-pi/4 + k * pi/(2N)) of the cell edges of a face, with tan(+-pi/4) = +-1 and tan(0) = 0 stored exactly"""
    k = np.arange(N + 1)
    t = np.tan(-np.pi / 4 + k * (np.pi / (2 * N)))
    t[0], t[N] = -1., 1.
    if N % 2 == 0:
        t[N // 2] = 0.
    return t


def _latlon_of(p):
    n = p / np.linalg.norm(p, axis=-1, keepdims=True)
    lat = np.rad2deg(np.arcsin(np.clip(n[..., 2], -1., 1.)))
    lon = np.mod(np.rad2deg(np.arctan2(n[..., 1], n[..., 0])), 360.)
    return lat, np.where(lon >= 360., 0., lon)


def _unit(lat, lon):
    la, lo = np.deg2rad(np.asarray(lat, np.float64)), np.deg2rad(np.asarray(lon, np.float64))
    return np.stack([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)], axis=-1)


def _corner_area(x, y):
    return np.arctan(x * y / np.sqrt(1. + x * x + y * y))


class CubeSphereGrid(object):
    """
    Equiangular gnomonic cubed sphere of N x N cells per face, cells (face, height, width) in face-major order.

    :param N: cells along a face side
    :param rotation: 3 x 3 orthogonal matrix applied to the face frames (determinant -1: a mirrored grid), or None
    """

    def __init__(self, N, rotation=None):
        self.N = int(N)
        if self.N < 1:
            raise ValueError('N = %d must be positive' % self.N)
        fr = default_frames()
        if rotation is not None:
            R = np.asarray(rotation, dtype=np.float64)
            if R.shape != (3, 3) or not np.allclose(R @ R.T, np.eye(3), atol=1e-9):
                raise ValueError('rotation must be a 3 x 3 orthogonal matrix')
            fr = fr @ R.T
        self.rotation = None if rotation is None else R
        self.frames = fr
        self.tangents = line_tangents(self.N)
        self.shape = (6, self.N, self.N)
        self.n_cells = 6 * self.N * self.N

    def points(self, f, i, j):
        """unit vectors at fractional cell coordinates (i: height, j: width) of faces f (arrays of one shape)"""
        h = np.pi / (2 * self.N)
        f = np.asarray(f)
        ta = np.tan(-np.pi / 4 + np.asarray(j, np.float64) * h)[..., None]
        tb = np.tan(-np.pi / 4 + np.asarray(i, np.float64) * h)[..., None]
        p = self.frames[f, 0] + ta * self.frames[f, 1] + tb * self.frames[f, 2]
        return p / np.linalg.norm(p, axis=-1, keepdims=True)

    @property
    def centres(self):
        """(6, N, N, 3) unit vectors of the cell centres"""
        f, i, j = np.meshgrid(np.arange(6), np.arange(self.N) + 0.5, np.arange(self.N) + 0.5, indexing='ij')
        return self.points(f, i, j)

    @property
    def lat(self):
        return _latlon_of(self.centres)[0]

    @property
    def lon(self):
        return _latlon_of(self.centres)[1]

    @property
    def area(self):
        t = self.tangents
        G = _corner_area(t[None, :], t[:, None])                          # [height line, width line]
        a = G[1:, 1:] - G[1:, :-1] - G[:-1, 1:] + G[:-1, :-1]
        return np.broadcast_to(a, (6, self.N, self.N)).copy()

    @classmethod
    def from_centres(cls, lat, lon):
        """The grid whose cell centres are the given (6, N, N) lat / lon in degrees: the rotation (or mirror) comes from an
        orthogonal Procrustes fit against the default grid.  ValueError when the centres are not such a grid."""
        lat, lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
        if lat.shape != lon.shape or lat.size % 6:
            raise ValueError('lat and lon must both hold 6 N^2 cell centres, got shapes %s and %s' % (lat.shape, lon.shape))
        N = int(round(np.sqrt(lat.size // 6)))
        if 6 * N * N != lat.size or N < 1:
            raise ValueError('%d cell centres are not 6 N^2' % lat.size)
        Q = _unit(lat.ravel(), lon.ravel())
        P = cls(N).centres.reshape(-1, 3)
        U, _, Vt = np.linalg.svd(Q.T @ P)
        R = U @ Vt
        res = float(np.abs(Q - P @ R.T).max())
        if not res <= _PROCRUSTES_TOL:
            raise ValueError('the centres are not those of an equiangular cubed sphere in (face, height, width) order: the '
                             'best orthogonal fit leaves a residual of %.3g' % res)
        return cls(N, rotation=R)


class LatLonGrid(object):
    """
    Regular lat-lon grid of n_lat x n_lon cells, lat-major, from its cell edges in degrees.

    :param lat_edges: n_lat + 1 strictly monotone latitudes within [-90, 90], ascending or descending
    :param lon_edges: n_lon + 1 ascending longitudes that span exactly 360 degrees (n_lon >= 2)
    """

    def __init__(self, lat_edges, lon_edges, lat=None, lon=None):
        le, lo = np.asarray(lat_edges, np.float64).ravel(), np.asarray(lon_edges, np.float64).ravel()
        if le.size < 2 or not (np.all(np.diff(le) > 0) or np.all(np.diff(le) < 0)):
            raise ValueError('latitude edges must be strictly monotone')
        if le.min() < -90. or le.max() > 90.:
            raise ValueError('latitude edges must lie within [-90, 90]')
        if lo.size < 3 or not np.all(np.diff(lo) > 0):
            raise ValueError('longitude edges must ascend and bound at least 2 cells')
        if abs((lo[-1] - lo[0]) - 360.) > 1e-9:
            raise ValueError('longitude edges must span exactly 360 degrees, not %r' % (lo[-1] - lo[0]))
        self.lat_edges, self.lon_edges = le, lo
        self.n_lat, self.n_lon = le.size - 1, lo.size - 1
        self.shape = (self.n_lat, self.n_lon)
        self.n_cells = self.n_lat * self.n_lon
        self.lat = 0.5 * (le[:-1] + le[1:]) if lat is None else np.asarray(lat, np.float64).copy()
        self.lon = 0.5 * (lo[:-1] + lo[1:]) if lon is None else np.asarray(lon, np.float64).copy()
        s = np.sin(np.deg2rad(le))
        s[le == 90.], s[le == -90.] = 1., -1.
        self.sin_lat_edges = s
        self.lon_edges_rad = np.deg2rad(lo)
        self.lon_edges_rad[-1] = self.lon_edges_rad[0] + 2 * np.pi

    @classmethod
    def cells(cls, n_lat, n_lon, inverse_lat=False, lon_begin=0.):
        """n_lat x n_lon equal cells over the sphere; latitudes descend from 90 with inverse_lat; lon_begin is the first edge"""
        n_lat, n_lon = int(n_lat), int(n_lon)
        le = -90. + 180. * np.arange(n_lat + 1) / n_lat
        le[-1] = 90.
        lo = float(lon_begin) + 360. * np.arange(n_lon + 1) / n_lon
        return cls(le[::-1] if inverse_lat else le, lo)

    @classmethod
    def from_centres(cls, lat, lon):
        """edges midway between the given centres, clipped at +-90: a centre on a pole gets a half cell"""
        lat, lon = np.asarray(lat, np.float64).ravel(), np.asarray(lon, np.float64).ravel()
        if lat.size < 2 or lon.size < 2:
            raise ValueError('at least 2 latitudes and 2 longitudes are needed')
        mid = 0.5 * (lat[:-1] + lat[1:])
        le = np.clip(np.r_[lat[0] - 0.5 * (lat[1] - lat[0]), mid, lat[-1] + 0.5 * (lat[-1] - lat[-2])], -90., 90.)
        mid = 0.5 * (lon[:-1] + lon[1:])
        first = lon[0] - 0.5 * (lon[1] - lon[0])
        return cls(le, np.r_[first, mid, first + 360.], lat=lat, lon=lon)

    @property
    def area(self):
        return np.abs(np.diff(self.sin_lat_edges))[:, None] * np.diff(self.lon_edges_rad)[None, :]
