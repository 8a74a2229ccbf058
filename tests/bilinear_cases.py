"""
The cubes and point sets shared by the bilinear sampling tests (tests/test_bilinear.py, tests/test_gpu_bilinear.py), the host
twin's result for each, computed once, and the property checks both files run.  No tests here.

Point sets per cube:
    interior: for every dual face 6 points made from (s, t) or barycentric coordinates drawn in [0.05, 0.95], put through the
        defining equation and normalised -- the containing face and the weights are known in closed form;
    boundary: all cell centres, the mid-points of all dual sides, the 8 cube vertices, points on the 12 cube edges, both poles
        at several longitudes and the longitudes 0, 360, -180 and 720.5.
"""
import functools

import numpy as np

CUBES = {'N1': (1, False), 'N2': (2, False), 'N3': (3, False), 'N5': (5, False), 'N8': (8, False), 'N5_mirrored': (5, True)}
PER_FACE = 6


def rotation():
    """the seeded mirrored rotation of tests/test_gpu_overlap.py"""
    rng = np.random.default_rng(11)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) > 0:
        q[:, 0] = -q[:, 0]
    return q


@functools.lru_cache(maxsize=None)
def cube(name):
    from DLWP.remap import CubeSphereGrid
    N, mirrored = CUBES[name]
    return CubeSphereGrid(N, rotation=rotation() if mirrored else None)


def latlon_of(p):
    p = p / np.linalg.norm(p, axis=-1, keepdims=True)
    return np.rad2deg(np.arcsin(np.clip(p[..., 2], -1., 1.))), np.rad2deg(np.arctan2(p[..., 1], p[..., 0]))


def unit(lat, lon):
    la, lo = np.deg2rad(np.asarray(lat, np.float64)), np.deg2rad(np.asarray(lon, np.float64))
    return np.stack([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)], axis=-1)


def field(p):
    """the test field x y + z.  Its gradient (y, x, 1) has norm sqrt(x^2 + y^2 + 1) <= sqrt(2) on the unit sphere."""
    return p[..., 0] * p[..., 1] + p[..., 2]


LIPSCHITZ = np.sqrt(2.)


@functools.lru_cache(maxsize=None)
def interior(name):
    """(lat, lon, cells (n, 4) with -1 in a triangle's fourth slot, weights (n, 4)) in the cells' order of dual_faces"""
    from DLWP.remap.bilinear import dual_faces
    cb = cube(name)
    V = cb.centres.reshape(-1, 3)
    quads, tris = dual_faces(cb)
    rng = np.random.default_rng(100 + cb.N)
    s, t = rng.uniform(0.05, 0.95, (2, quads.shape[0], PER_FACE))
    wq = np.stack([(1 - s) * (1 - t), s * (1 - t), s * t, (1 - s) * t], axis=-1)            # (Q, P, 4)
    pq = np.einsum('qpk,qkc->qpc', wq, V[quads])
    b = rng.uniform(0.05, 0.95, (tris.shape[0], PER_FACE, 3))
    b /= b.sum(axis=-1, keepdims=True)
    pt = np.einsum('qpk,qkc->qpc', b, V[tris])
    wt = np.concatenate([b, np.zeros(b.shape[:2] + (1,))], axis=-1)
    ct = np.concatenate([tris, np.full((tris.shape[0], 1), -1)], axis=1)
    cells = np.concatenate([np.repeat(quads, PER_FACE, axis=0), np.repeat(ct, PER_FACE, axis=0)])
    w = np.concatenate([wq.reshape(-1, 4), wt.reshape(-1, 4)])
    lat, lon = latlon_of(np.concatenate([pq.reshape(-1, 3), pt.reshape(-1, 3)]))
    for a in (lat, lon, cells, w):
        a.setflags(write=False)
    return lat, lon, cells, w


@functools.lru_cache(maxsize=None)
def boundary(name):
    """(lat, lon, own): own is the cell of which the point is the centre, or -1"""
    from DLWP.remap.bilinear import dual_faces
    cb = cube(name)
    V = cb.centres.reshape(-1, 3)
    quads, tris = dual_faces(cb)
    sides = set()
    for faces in (quads, tris):
        for fc in faces:
            for k in range(len(fc)):
                sides.add((min(fc[k], fc[(k + 1) % len(fc)]), max(fc[k], fc[(k + 1) % len(fc)])))
    sides = np.array(sorted(sides))
    mids = V[sides[:, 0]] + V[sides[:, 1]]
    fr = cb.frames
    verts = np.array([fr[0, 0] * sx + fr[1, 0] * sy + fr[5, 0] * sz for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
    y = np.array([-1., -0.77, -0.3, 0., 0.123, 0.5, 0.99])
    edges = [fr[f, 0] + sg * fr[f, a] + y[:, None] * fr[f, 3 - a] for f in range(6) for a in (1, 2) for sg in (-1, 1)]
    lat, lon = latlon_of(np.concatenate([V, mids, verts] + edges))
    own = np.full(lat.size, -1)
    own[:V.shape[0]] = np.arange(V.shape[0])
    pole_lon = np.array([0., 45., 90., 180., 270., 359.9, -33.])
    wrap_lon = np.array([0., 360., -180., 720.5])
    wrap_lat = np.array([-90., -35.26, 0., 12.5, 45., 90.])
    lat = np.concatenate([lat, np.full(7, 90.), np.full(7, -90.), np.repeat(wrap_lat, 4)])
    lon = np.concatenate([lon, pole_lon, pole_lon, np.tile(wrap_lon, 6)])
    own = np.concatenate([own, np.full(lat.size - own.size, -1)])
    for a in (lat, lon, own):
        a.setflags(write=False)
    return lat, lon, own


@functools.lru_cache(maxsize=None)
def host_weights(name, which):
    """(col, w) of the host twin on the interior or boundary set; treat as read-only"""
    from DLWP.remap.bilinear import point_weights
    lat, lon = (interior if which == 'interior' else boundary)(name)[:2]
    out = point_weights(cube(name), lat, lon)
    for a in out:
        a.setflags(write=False)
    return out


def check_properties(cb, lat, lon, col, w, own=None):
    """The properties every answer must have, whichever of two neighbouring dual faces a boundary point was given to.
    Returns the largest residuals (sum, direction) for printing."""
    V = cb.centres.reshape(-1, 3)
    P = unit(lat, np.mod(lon, 360.))
    assert col.shape == w.shape == (P.shape[0], 4)
    assert col.min() >= 0 and col.max() < cb.n_cells
    assert np.all(w >= 0)
    res_sum = float(np.abs(w.sum(axis=1) - 1.).max())
    assert res_sum <= 1e-14
    Q = np.einsum('nk,nkc->nc', w, V[col])
    res_dir = float(np.linalg.norm(np.cross(P, Q), axis=1).max())
    assert res_dir <= 1e-12
    assert np.all(np.einsum('nc,nc->n', Q, P) > 0)
    tri = col[:, 3] == col[:, 2]
    assert np.all(w[tri, 3] == 0.)
    assert cb.N > 1 or tri.all()
    if own is not None:
        at = np.nonzero(own >= 0)[0]
        w_own = np.where(col[at] == own[at, None], w[at], 0.).sum(axis=1)
        assert np.all(w_own >= 1. - 1e-12)
    return res_sum, res_dir


def sample(cb, col, w):
    return (w * field(cb.centres.reshape(-1, 3))[col]).sum(axis=1)
