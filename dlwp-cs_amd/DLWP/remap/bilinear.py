"""
Sampling a cubed-sphere field at arbitrary points: the bilinear map on the dual mesh of the cube.  This module
is the numpy twin of csrc/bilinear.hip and states the maths; `point_weights(..., device=...)` runs the kernel instead
(dlwpcs_cube_bilinear).

The dual mesh of an equiangular cube of N x N cells per face has the 6 N^2 cell centres as vertices and three kinds of faces,
all bounded by great-circle arcs between centres:
    (a) per cube face the (N - 1)^2 quadrilaterals of the centres (i, j), (i, j + 1), (i + 1, j + 1), (i + 1, j).  Their
        sides are coordinate lines of the face (a line of constant equiangular coordinate is a great circle), so they are the
        rectangles [j, j + 1] x [i, i + 1] in the fractional cell coordinates of the centres;
    (b) per cube edge the N - 1 quadrilaterals of an edge strip: the border cells k and k + 1 of one face and the two cells
        that face them across the edge.  The arcs between a border cell and the cell facing it are the strip's rungs;
    (c) per cube vertex the triangle of the three corner cells.
For a point P in a quadrilateral V0..V3 the weights are the bilinear factors of the (s, t) with
(1-s)(1-t) V0 + s(1-t) V1 + s t V2 + (1-s) t V3 = lambda P; in a triangle they are the barycentric coordinates of the radial
projection of P onto the triangle's plane.  Along a side of a dual face the weights depend on the side's two ends only (they
are linear along the chord), so the interpolant is continuous over the whole sphere.

A point is located in the face whose centre it is nearest to.  Inside the rectangle of that face's centres it lies in a
quadrilateral of kind (a).  Outside, the rungs decide: they are not coordinate lines of either face, so the strip is walked
from the cell the along-edge coordinate names, by the sign of P . (V_in x V_out), until P lies between two rungs; a point
beyond the last rung of both strips it could belong to lies in the corner's triangle.
"""
import numpy as np

from ..labelled import is_tensor as _is_tensor
from .grid import CubeSphereGrid, LatLonGrid, default_frames

SIDES = ('west', 'east', 'south', 'north')       # side 0: width index 0, 1: width N - 1, 2: height 0, 3: height N - 1
NEWTON_STEPS = 12                                # fixed: the same call gives the same bits
_EDGES = None


def cube_edges():
    """
    (6, 4, 3) int32: for every face and side (SIDES) the neighbour face, the neighbour's side that is the same cube edge, and
    1 when the position along the edge runs the other way there.  Derived from default_frames() by geometry; a rotation or
    mirror of the grid moves all frames alike and does not change it.  Computed once; the array is read-only.
    """
    global _EDGES
    if _EDGES is not None:
        return _EDGES
    fr = default_frames()
    out_dir = lambda f, s: (-fr[f, 1], fr[f, 1], -fr[f, 2], fr[f, 2])[s]
    along = lambda f, s: fr[f, 2] if s < 2 else fr[f, 1]
    edge = np.zeros((6, 4, 3), dtype=np.int32)
    for f in range(6):
        for s in range(4):
            mid = fr[f, 0] + out_dir(f, s)
            hit = [(g, t) for g in range(6) for t in range(4) if g != f and np.allclose(fr[g, 0] + out_dir(g, t), mid)]
            assert len(hit) == 1
            g, t = hit[0]
            edge[f, s] = (g, t, int(np.dot(along(f, s), along(g, t)) < 0))
    edge.setflags(write=False)
    _EDGES = edge
    return edge


def _border(N, side, k):
    """(i, j) of border cell k along a side"""
    side, k = np.asarray(side), np.asarray(k)
    z, top = np.zeros_like(k), np.full_like(k, N - 1)
    i = np.where(side == 2, z, np.where(side == 3, top, k))
    j = np.where(side == 0, z, np.where(side == 1, top, k))
    return i, j


def _facing(N, edge, f, side, k):
    """(face, i, j) of the cell that faces border cell k of (f, side) across the cube edge"""
    e = edge[f, side]
    g, t = e[..., 0], e[..., 1]
    i, j = _border(N, t, np.where(e[..., 2] == 1, N - 1 - k, k))
    return g, i, j


def _flat(N, f, i, j):
    return (f * N + i) * N + j


def dual_faces(cube):
    """
    The dual mesh as index arrays of cube cells (f N + i) N + j: (quads (6 (N-1)^2 + 12 (N-1), 4) in cyclic order, triangles
    (8, 3)).  For tests and documentation.
    """
    N = cube.N if isinstance(cube, CubeSphereGrid) else int(cube)
    edge = cube_edges()
    quads = []
    for f in range(6):
        for i in range(N - 1):
            for j in range(N - 1):
                quads.append([_flat(N, f, i, j), _flat(N, f, i, j + 1), _flat(N, f, i + 1, j + 1), _flat(N, f, i + 1, j)])
    tris = set()
    for f in range(6):
        for s in range(4):
            g, t, _ = edge[f, s]
            if (g, t) < (f, s):                      # every cube edge once
                continue
            for k in range(N - 1):
                cells = []
                for kk in (k, k + 1):
                    i, j = _border(N, s, kk)
                    go, io, jo = _facing(N, edge, f, s, kk)
                    cells.append((_flat(N, f, int(i), int(j)), _flat(N, int(go), int(io), int(jo))))
                quads.append([cells[0][0], cells[0][1], cells[1][1], cells[1][0]])
        for sa in (0, 1):
            for sb in (2, 3):
                tris.add(tuple(sorted(_corner_cells(N, edge, f, sa, sb))))
    return np.array(quads, dtype=np.int64).reshape(-1, 4), np.array(sorted(tris), dtype=np.int64).reshape(-1, 3)


def _corner_cells(N, edge, f, sa, sb):
    """the three corner cells at the (sa in west / east, sb in south / north) corner of face f, this face's first"""
    ka, kb = (0 if sa == 0 else N - 1), (0 if sb == 2 else N - 1)
    i, j = kb, ka
    g2, i2, j2 = _facing(N, edge, f, sa, kb)         # across the west / east side: position along it is the height index
    g3, i3, j3 = _facing(N, edge, f, sb, ka)
    return _flat(N, f, i, j), _flat(N, int(g2), int(i2), int(j2)), _flat(N, int(g3), int(i3), int(j3))


def unit_vectors(lat, lon):
    """(n, 3) unit vectors of points given in degrees; the longitude is wrapped into [0, 360) first (exactly)"""
    la = np.deg2rad(np.asarray(lat, np.float64).ravel())
    lo = np.deg2rad(np.mod(np.asarray(lon, np.float64).ravel(), 360.))
    c = np.cos(la)
    return np.stack([c * np.cos(lo), c * np.sin(lo), np.sin(la)], axis=-1)


def _det(a, b, c):
    return np.einsum('...k,...k->...', a, np.cross(b, c))


def _tangents(P):
    """two unit vectors that span the plane orthogonal to P: along P x (the axis of P's smallest component) and P x that"""
    ax = np.zeros_like(P)
    ax[np.arange(P.shape[0]), np.argmin(np.abs(P), axis=1)] = 1.
    u1 = np.cross(P, ax)
    u1 /= np.linalg.norm(u1, axis=1, keepdims=True)
    return u1, np.cross(P, u1)


def _solve_quad(P, V, s, t):
    """Newton for (s, t) of the quadrilateral V (n, 4, 3) from the given guess, NEWTON_STEPS steps, clipped to [0, 1] at the end"""
    u1, u2 = _tangents(P)
    A, B, C, D = V[:, 0], V[:, 1] - V[:, 0], V[:, 3] - V[:, 0], V[:, 0] - V[:, 1] + V[:, 2] - V[:, 3]
    dot = lambda x, y: np.einsum('nk,nk->n', x, y)
    a1, b1, c1, d1 = dot(A, u1), dot(B, u1), dot(C, u1), dot(D, u1)
    a2, b2, c2, d2 = dot(A, u2), dot(B, u2), dot(C, u2), dot(D, u2)
    s, t = s.copy(), t.copy()
    for _ in range(NEWTON_STEPS):
        F1 = a1 + s * b1 + t * c1 + s * t * d1
        F2 = a2 + s * b2 + t * c2 + s * t * d2
        j11, j12, j21, j22 = b1 + t * d1, c1 + s * d1, b2 + t * d2, c2 + s * d2
        det = j11 * j22 - j12 * j21
        s, t = s - (F1 * j22 - F2 * j12) / det, t - (F2 * j11 - F1 * j21) / det
    s, t = np.clip(s, 0., 1.), np.clip(t, 0., 1.)
    return np.stack([(1. - s) * (1. - t), s * (1. - t), s * t, (1. - s) * t], axis=1)


def _solve_tri(P, V):
    """barycentric weights of the radial projection of P on the triangle V (n, 3, 3), negative rounding clipped, sum 1"""
    b = np.stack([_det(P, V[:, 1], V[:, 2]), _det(V[:, 0], P, V[:, 2]), _det(V[:, 0], V[:, 1], P)], axis=1)
    b = b / _det(V[:, 0], V[:, 1], V[:, 2])[:, None]
    b = np.maximum(b, 0.)
    return b / (b[:, 0] + b[:, 1] + b[:, 2])[:, None]


def _host_weights(cube, P):
    N, fr = cube.N, cube.frames
    n = P.shape[0]
    edge = cube_edges()
    h = np.pi / (2 * N)
    f = np.argmax(P @ fr[:, 0].T, axis=1)
    e0, eu, ev = fr[f, 0], fr[f, 1], fr[f, 2]
    dot = lambda x, y: np.einsum('nk,nk->n', x, y)
    p0 = dot(P, e0)
    a = (np.arctan2(dot(P, eu), p0) + np.pi / 4) / h - 0.5          # width, in cells from the first centre
    b = (np.arctan2(dot(P, ev), p0) + np.pi / 4) / h - 0.5          # height
    col = np.zeros((n, 4), dtype=np.int64)
    w = np.zeros((n, 4))
    done = np.zeros(n, dtype=bool)

    def centres(ff, i, j):
        return cube.points(ff, np.asarray(i) + 0.5, np.asarray(j) + 0.5)

    inside = (a >= 0) & (a <= N - 1) & (b >= 0) & (b <= N - 1) if N >= 2 else np.zeros(n, dtype=bool)
    idx = np.nonzero(inside)[0]
    if idx.size:
        j0 = np.clip(np.floor(a[idx]), 0, N - 2).astype(np.int64)
        i0 = np.clip(np.floor(b[idx]), 0, N - 2).astype(np.int64)
        ff = f[idx]
        cells = [(i0, j0), (i0, j0 + 1), (i0 + 1, j0 + 1), (i0 + 1, j0)]
        V = np.stack([centres(ff, i, j) for i, j in cells], axis=1)
        col[idx] = np.stack([_flat(N, ff, i, j) for i, j in cells], axis=1)
        w[idx] = _solve_quad(P[idx], V, a[idx] - j0, b[idx] - i0)
        done[idx] = True

    if N >= 2:
        for side in range(4):
            beyond = (a < 0, a > N - 1, b < 0, b > N - 1)[side]
            idx = np.nonzero(beyond & ~done)[0]
            if not idx.size:
                continue
            ff, Pi = f[idx], P[idx]
            c = (b if side < 2 else a)[idx]
            sd = np.full(idx.size, side)
            along = fr[ff, 2] if side < 2 else fr[ff, 1]
            outward = (-fr[ff, 1], fr[ff, 1], -fr[ff, 2], fr[ff, 2])[side]
            sgn = _det(along, fr[ff, 0], outward)                   # orientation of a rung's triple product (mirrored grids)

            def rung(m):
                """P's side of rung m, positive towards larger positions; the rung's two centres and cells"""
                i, j = _border(N, sd, m)
                g, io, jo = _facing(N, edge, ff, sd, m)
                Vi, Vo = centres(ff, i, j), centres(g, io, jo)
                return sgn * _det(Pi, Vi, Vo), Vi, Vo, _flat(N, ff, i, j), _flat(N, g, io, jo)

            k = np.clip(np.floor(c), 0, N - 2).astype(np.int64)
            live = np.ones(idx.size, dtype=bool)                    # still walking, and inside the strip
            heading = np.zeros(idx.size, dtype=np.int64)            # the walk never turns back: a point on a rung stays put
            for _ in range(N + 1):
                kc = np.clip(k, 0, N - 2)
                lo, hi = rung(kc)[0], rung(kc + 1)[0]
                step = np.where((lo < 0) & (heading <= 0), -1, np.where((hi > 0) & (heading >= 0), 1, 0)) * live
                heading = np.where(step != 0, step, heading)
                k = k + step
                live &= (k >= 0) & (k <= N - 2)
                if not np.any(step[live] != 0):
                    break
            settled = live & (step == 0)
            sel = np.nonzero(settled)[0]
            if sel.size:
                ff, Pi, sd, sgn = ff[sel], Pi[sel], sd[sel], sgn[sel]        # (rung reads these)
                ks = k[sel]
                _, Vi0, Vo0, ci0, co0 = rung(ks)
                _, Vi1, Vo1, ci1, co1 = rung(ks + 1)
                V = np.stack([Vi0, Vo0, Vo1, Vi1], axis=1)
                col[idx[sel]] = np.stack([ci0, co0, co1, ci1], axis=1)
                w[idx[sel]] = _solve_quad(Pi, V, np.full(sel.size, 0.25), np.clip(c[sel] - ks, 0., 1.))
                done[idx[sel]] = True

    idx = np.nonzero(~done)[0]
    if idx.size:
        ff = f[idx]
        sa = np.where(a[idx] < 0.5 * (N - 1), 0, 1)
        sb = np.where(b[idx] < 0.5 * (N - 1), 2, 3)
        ka, kb = np.where(sa == 0, 0, N - 1), np.where(sb == 2, 0, N - 1)
        g2, i2, j2 = _facing(N, edge, ff, sa, kb)
        g3, i3, j3 = _facing(N, edge, ff, sb, ka)
        V = np.stack([centres(ff, kb, ka), centres(g2, i2, j2), centres(g3, i3, j3)], axis=1)
        c3 = _flat(N, g3, i3, j3)
        col[idx] = np.stack([_flat(N, ff, kb, ka), _flat(N, g2, i2, j2), c3, c3], axis=1)
        w[idx, :3] = _solve_tri(P[idx], V)
        w[idx, 3] = 0.
    return col.astype(np.int32), w


def _checked_points(lat, lon):
    lat, lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
    if lat.shape != lon.shape:
        raise ValueError('lat and lon must have one shape, got %s and %s' % (lat.shape, lon.shape))
    if not (np.all(np.isfinite(lat)) and np.all(np.isfinite(lon))):
        raise ValueError('lat and lon must be finite')
    if lat.size and np.abs(lat).max() > 90.:
        raise ValueError('latitudes must lie within [-90, 90]')
    return lat.ravel(), lon.ravel()


def point_weights(cube, lat, lon, device=None):
    """
    The cells and weights that sample a field on `cube` at the points (lat, lon) in degrees (any one shape, flattened in C
    order; any finite longitude; |lat| <= 90, otherwise ValueError, as for non-finite input).

    :return: (col (n, 4) int32 cube cells (f N + i) N + j, w (n, 4) float64): non-negative, each row sums to 1.  A point in a
        corner triangle repeats its third cell in the fourth slot with weight exactly 0.0.
    device=None: this module.  A HIP device: the dlwpcs_cube_bilinear kernel; lat / lon that are tensors on that device stay
    there, and so does the result (two tensors).
    """
    if device is not None:
        from .. import ops
        return ops.cube_bilinear(cube, lat, lon, device)
    lat, lon = _checked_points(lat, lon)
    return _host_weights(cube, unit_vectors(lat, lon))


def bilinear_map(cube, lat=None, lon=None, *, latlon=None, device=None):
    """
    The bilinear sampling map from `cube` as an OfflineMap of four entries per row: to the cell centres of a LatLonGrid
    (`latlon`: dst_kind 'latlon', lat_b / lon_b set, so CubeSphereRemap.inverse_remap_forecast takes it), or to the points
    (lat, lon) in degrees (dst_kind 'cells' of shape (n,), yc_b / xc_b the points).  device: as point_weights.
    """
    from .offline_map import OfflineMap
    if not isinstance(cube, CubeSphereGrid):
        raise TypeError('cube must be a DLWP.remap.CubeSphereGrid')
    if latlon is not None:
        if lat is not None or lon is not None:
            raise ValueError('give either latlon= or the points lat, lon')
        if not isinstance(latlon, LatLonGrid):
            raise TypeError('latlon must be a DLWP.remap.LatLonGrid')
        yc, xc = (g.ravel() for g in np.meshgrid(latlon.lat, latlon.lon, indexing='ij'))
        dims, as_cells = np.array([latlon.n_lon, latlon.n_lat], np.int32), False
    else:
        if lat is None or lon is None:
            raise ValueError('bilinear_map needs the points lat and lon, or latlon=')
        if device is not None and (_is_tensor(lat) or _is_tensor(lon)):
            lat, lon = (np.asarray(x.detach().cpu().numpy() if _is_tensor(x) else x, np.float64) for x in (lat, lon))
        yc, xc = _checked_points(lat, lon)
        dims, as_cells = np.array([yc.size], np.int32), True
    col, w = point_weights(cube, yc, xc, device=device)
    if device is not None:
        col, w = col.cpu().numpy(), w.cpu().numpy()
    n = yc.size
    row = np.repeat(np.arange(1, n + 1, dtype=np.int64), 4)
    return OfflineMap(row, col.ravel().astype(np.int64) + 1, w.ravel(), cube.n_cells, n,
                      src_grid_dims=np.array([cube.n_cells], np.int32), dst_grid_dims=dims, yc_a=cube.lat.ravel(),
                      xc_a=cube.lon.ravel(), yc_b=yc, xc_b=xc, dst_cells=as_cells)
