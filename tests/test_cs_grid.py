"""
The closed-form grids of map generation (DLWP.remap.grid): the cubed sphere's geometry against the padding layer's layout, its
cell areas and face centres, recovery of a rotated or mirrored grid from its cell centres, and the lat-lon grid's edges.
"""
import numpy as np
import pytest

from oracle import cs_oracle as orc
from DLWP.remap import CubeSphereGrid, LatLonGrid


@pytest.mark.parametrize('N', [4, 5, 8])
def test_halo_cells_are_the_geometric_neighbours(N):
    """every non-corner halo cell of CubeSpherePadding2D(1) holds the centre nearest to the face's own grid continued one cell
    outward: the frames are the layout the padding layer encodes"""
    g = CubeSphereGrid(N)
    cen = g.centres
    pad = orc.cs_pad(cen[None], 1, 'channels_last')
    pad = np.asarray(pad)[0]
    assert pad.shape == (6, N + 2, N + 2, 3)
    flat = cen.reshape(-1, 3)
    bad = checked = 0
    for f in range(6):
        for a in range(N + 2):
            for b in range(N + 2):
                edge_a, edge_b = a in (0, N + 1), b in (0, N + 1)
                if edge_a == edge_b:                           # interior or corner
                    continue
                p = g.points(f, a - 0.5, b - 0.5)
                want = flat[np.argmax(flat @ p)]
                checked += 1
                bad += not np.array_equal(pad[f, a, b], want)
    assert checked == 6 * 4 * N
    assert bad == 0


@pytest.mark.parametrize('N', [1, 4, 5, 8, 48])
def test_areas(N):
    g = CubeSphereGrid(N)
    a = g.area
    assert a.shape == (6, N, N) and (a > 0).all()
    assert abs(a.sum() / (4 * np.pi) - 1.) < 1e-13
    # the symmetries of a face, and all faces alike.  An area is a sum of four arctangents of at most pi / 6, each good to a
    # few ulp of 0.5: 16 * 2^-52 absolute, whatever the cell's size
    tol = 16 * np.finfo(np.float64).eps
    for f in range(6):
        assert np.array_equal(a[f], a[0])
        for s in (a[f].T, a[f][::-1], a[f][:, ::-1]):
            assert np.abs(a[f] - s).max() <= tol


@pytest.mark.parametrize('N', [3, 4])
def test_face_centres(N):
    g = CubeSphereGrid(N)
    h = (N - 1) / 2.
    p = g.points(np.arange(6), np.full(6, N / 2.), np.full(6, N / 2.))
    lat = np.rad2deg(np.arcsin(p[:, 2]))
    lon = np.mod(np.rad2deg(np.arctan2(p[:, 1], p[:, 0])), 360.)
    assert np.allclose(lat, [0, 0, 0, 0, -90, 90], atol=1e-12)
    assert np.allclose(lon[:4], [0, 90, 180, 270], atol=1e-12)
    assert g.lat.shape == (6, N, N) and (g.lon >= 0).all() and (g.lon < 360).all()
    if N % 2:                                                 # odd N: the middle cell's centre is the face centre
        m = int(h)
        assert np.allclose(g.lat[:, m, m], [0, 0, 0, 0, -90, 90], atol=1e-12)
        assert np.allclose(g.lon[:4, m, m], [0, 90, 180, 270], atol=1e-12)
    assert (g.lat[5] > 30).all() and (g.lat[4] < -30).all()


def test_shared_edges_are_exact():
    for N in (4, 5):
        t = CubeSphereGrid(N).tangents
        assert t[0] == -1. and t[-1] == 1.
        if N % 2 == 0:
            assert t[N // 2] == 0.


def _random_rotation(rng, mirror):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if (np.linalg.det(q) < 0) != mirror:
        q[:, 0] = -q[:, 0]
    return q


@pytest.mark.parametrize('mirror', [False, True])
def test_from_centres_recovers_rotation(mirror):
    rng = np.random.default_rng(5 + mirror)
    R = _random_rotation(rng, mirror)
    assert (np.linalg.det(R) < 0) == mirror
    g = CubeSphereGrid(6, rotation=R)
    back = CubeSphereGrid.from_centres(g.lat, g.lon)
    assert back.N == 6
    assert np.abs(back.rotation - R).max() < 1e-12
    assert np.abs(back.frames - g.frames).max() < 1e-12
    assert np.abs(CubeSphereGrid.from_centres(CubeSphereGrid(4).lat, CubeSphereGrid(4).lon).rotation - np.eye(3)).max() < 1e-12


def test_from_centres_refuses_other_grids():
    g = CubeSphereGrid(4)
    perm = np.random.default_rng(0).permutation(g.n_cells)
    with pytest.raises(ValueError):
        CubeSphereGrid.from_centres(g.lat.ravel()[perm], g.lon.ravel()[perm])
    with pytest.raises(ValueError):
        CubeSphereGrid.from_centres(g.lat[[0, 1, 2, 3, 5, 4]], g.lon[[0, 1, 2, 3, 5, 4]])      # polar faces swapped, not rotated
    with pytest.raises(ValueError):
        CubeSphereGrid.from_centres(np.zeros(7), np.zeros(7))


def test_latlon_grids():
    g = LatLonGrid.cells(6, 12, lon_begin=-15.)
    assert g.shape == (6, 12) and g.lat[0] == -75. and g.lon[0] == 0.
    assert g.sin_lat_edges[0] == -1. and g.sin_lat_edges[-1] == 1.
    assert abs(g.area.sum() / (4 * np.pi) - 1.) < 1e-14
    inv = LatLonGrid.cells(6, 12, inverse_lat=True)
    assert inv.lat[0] == 75. and np.allclose(inv.area, g.area[::-1], rtol=1e-15)
    era = LatLonGrid.from_centres(np.linspace(90, -90, 721), np.arange(1440) * 0.25)
    assert era.lat_edges[0] == 90. and era.lat_edges[1] == 89.875 and era.lat_edges[-1] == -90.
    assert era.lon_edges[0] == -0.125 and era.lat[0] == 90. and era.lon[1] == 0.25
    assert abs(era.area.sum() / (4 * np.pi) - 1.) < 1e-13
    # a pole-centred half cell: (1 - cos d) against (cos d - cos 3d), d = 0.125 degrees
    assert abs(era.area[0, 0] / era.area[1, 0] - 0.125) < 1e-5
    for bad in (([-90, 0, 0, 90], [0, 180, 360]), ([-91, 90], [0, 180, 360]), ([-90, 90], [0, 360]),
                ([-90, 90], [0, 180, 350]), ([-90, 90], [0, 200, 180, 360])):
        with pytest.raises(ValueError):
            LatLonGrid(*bad)
