"""
Areas of the intersections of lat-lon cells with cubed-sphere cells, in closed form and fp64: the matrix A[r, c] from which
both conservative maps are made.  This module is the numpy twin of csrc/overlap.hip, vectorised over the
candidate pairs; `overlap_areas(..., device=...)` runs the kernels instead (dlwpcs_overlap_count / dlwpcs_overlap_fill).

In (lambda, sin phi) area is d lambda * d sin phi and a lat-lon cell is a rectangle.  A cube cell is four half-spaces n.p >= 0.
A plane with n_z != 0 bounds the latitude by the curve tan phi = c cos(lambda - l*), from below when n_z > 0 and from above
when n_z < 0; sin phi on the curve has the antiderivative asin(c sin(lambda - l*) / sqrt(1 + c^2)).  A plane with n_z = 0
keeps the half circle cos(lambda - l*) >= 0.  The area is the integral over the cell's longitudes of
[min(s2, uppers) - max(s1, lowers)]+, cut at every longitude where the active bounds can change.
"""
import numpy as np

DUST = 1e-10                 # entries with A <= DUST * min(area_r, area_c) are cells that only share an edge: dropped
MERIDIAN_EPS = 1e-14         # |n_z| <= MERIDIAN_EPS * hypot(n_x, n_y): the plane holds the z axis
CAP_SLACK = 1e-9             # radians added to the bounding cap of a lat-lon cell and to its index ranges
N_BREAKS = 22                # 2 interval ends + 4 corners + 4 planes x 4
_CHUNK = 1 << 15


def _wrap(x):
    return x - (2 * np.pi) * np.round(x / (2 * np.pi))


def _cell_geometry(ll):
    """per lat-lon cell (flat, lat-major): s1 < s2, the centre longitude and half width in radians"""
    s = ll.sin_lat_edges
    s1, s2 = np.minimum(s[:-1], s[1:]), np.maximum(s[:-1], s[1:])
    lo = ll.lon_edges_rad
    lc, w = 0.5 * (lo[:-1] + lo[1:]), 0.5 * (lo[1:] - lo[:-1])
    rep = lambda a, lat: (np.repeat(a, ll.n_lon) if lat else np.tile(a, ll.n_lat))
    return rep(s1, True), rep(s2, True), rep(lc, False), rep(w, False)


def candidates(cube, ll):
    """
    (r, c): every pair of a lat-lon cell and a cube cell whose intersection may be non-empty, sorted by r, then c.  Per face
    the lat-lon cell is bounded by a cap about its centre that reaches its corners; the cap's extent in each of the face's two
    equiangular coordinates is an index range.
    """
    N, h = cube.N, np.pi / (2 * cube.N)
    s1, s2, lc, w = _cell_geometry(ll)
    p1, p2 = np.arcsin(s1), np.arcsin(s2)
    pc = 0.5 * (p1 + p2)
    q = np.stack([np.cos(pc) * np.cos(lc), np.cos(pc) * np.sin(lc), np.sin(pc)], axis=1)
    # the farthest points of the cell from its centre are its corners (the cell is at most 180 degrees wide)
    cw = np.cos(w)
    d = np.minimum(np.sin(pc) * s1 + np.cos(pc) * np.cos(p1) * cw, np.sin(pc) * s2 + np.cos(pc) * np.cos(p2) * cw)
    rho = np.arccos(np.clip(d, -1., 1.)) + CAP_SLACK
    srho = np.sin(rho)
    rr, cc = [], []
    for f in range(6):
        e0, eu, ev = cube.frames[f]
        rng = []
        for along, across in ((eu, ev), (ev, eu)):
            a0 = np.arctan2(q @ along, q @ e0)
            cel = np.sqrt(np.maximum(0., 1. - (q @ across) ** 2))
            full = (rho >= np.pi / 2) | (srho >= cel * (1. - 1e-12))
            dl = np.arcsin(np.minimum(1., srho / np.where(full, 1., cel))) + CAP_SLACK
            lo = np.where(full, 0, np.clip(np.floor((a0 - dl + np.pi / 4) / h), 0, N)).astype(np.int64)
            hi = np.where(full, N - 1, np.clip(np.floor((a0 + dl + np.pi / 4) / h), -1, N - 1)).astype(np.int64)
            rng.append((lo, hi))
        (j0, j1), (i0, i1) = rng
        nj, ni = np.maximum(j1 - j0 + 1, 0), np.maximum(i1 - i0 + 1, 0)
        cnt = ni * nj
        r = np.repeat(np.arange(cnt.size), cnt)
        k = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        njr = np.repeat(nj, cnt)
        i, j = np.repeat(i0, cnt) + k // np.maximum(njr, 1), np.repeat(j0, cnt) + k % np.maximum(njr, 1)
        rr.append(r)
        cc.append((f * N + i) * N + j)
    r, c = np.concatenate(rr), np.concatenate(cc)
    o = np.lexsort((c, r))
    return r[o], c[o]


def pair_areas(cube, ll, r, c):
    """A[r, c] for the given pairs (arrays of flat lat-lon cells and flat cube cells), fp64; 0 where they do not meet"""
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    out = np.empty(r.size)
    geo = _cell_geometry(ll)
    for a in range(0, r.size, _CHUNK):
        out[a:a + _CHUNK] = _pair_areas(cube, geo, r[a:a + _CHUNK], c[a:a + _CHUNK])
    return out


def _pair_areas(cube, geo, r, c):
    N, t = cube.N, cube.tangents
    s1, s2, lc, w = (g[r] for g in geo)
    f, i, j = c // (N * N), (c // N) % N, c % N
    e0, eu, ev = cube.frames[f, 0], cube.frames[f, 1], cube.frames[f, 2]
    xa, xb, ya, yb = t[j][:, None], t[j + 1][:, None], t[i][:, None], t[i + 1][:, None]
    n = np.stack([eu - xa * e0, xb * e0 - eu, ev - ya * e0, yb * e0 - ev], axis=1)            # (M, 4, 3)
    hyp, nz = np.hypot(n[..., 0], n[..., 1]), n[..., 2]
    merid = np.abs(nz) <= MERIDIAN_EPS * hyp
    lam = np.arctan2(n[..., 1], n[..., 0])
    cc = np.where(merid, 0., -hyp / np.where(merid, 1., nz))
    kk = cc / np.sqrt(1. + cc * cc)
    lower, upper = ~merid & (nz > 0), ~merid & (nz < 0)

    M = r.size
    br = np.full((M, N_BREAKS), np.nan)
    br[:, 0], br[:, 1] = -w, w
    for k, (x, y) in enumerate(((xa, ya), (xb, ya), (xa, yb), (xb, yb))):
        P = e0 + x * eu + y * ev
        ok = np.hypot(P[:, 0], P[:, 1]) > MERIDIAN_EPS * np.linalg.norm(P, axis=1)
        br[:, 2 + k] = np.where(ok, _wrap(np.arctan2(P[:, 1], P[:, 0]) - lc), np.nan)
    with np.errstate(divide='ignore', invalid='ignore'):
        for e, s in enumerate((s1, s2)):
            te = s / np.sqrt(1. - s * s)                                                      # +-inf at a pole
            ratio = te[:, None] / cc
            th = np.where(~merid & (np.abs(ratio) <= 1.), np.arccos(np.clip(ratio, -1., 1.)), np.nan)
            if e == 0:
                th = np.where(merid, np.pi / 2, th)
            for sg, sign in enumerate((1., -1.)):
                br[:, 6 + 4 * np.arange(4) + 2 * e + sg] = _wrap(lam + sign * th - lc[:, None])
    br = np.clip(np.where(np.isnan(br), w[:, None], br), -w[:, None], w[:, None])
    br.sort(axis=1)

    a, b = br[:, :-1], br[:, 1:]                                                              # (M, pieces)
    live = b > a
    m = 0.5 * (a + b)
    th = (m + lc[:, None])[:, :, None] - lam[:, None, :]                                      # (M, pieces, 4)
    cm = np.cos(th)
    live &= ~np.any(merid[:, None, :] & (cm < 0.), axis=2)
    u = cc[:, None, :] * cm
    sv = u / np.sqrt(1. + u * u)
    up = np.where(upper[:, None, :], sv, np.inf)
    lw = np.where(lower[:, None, :], sv, -np.inf)
    iu, il = np.argmin(up, axis=2), np.argmax(lw, axis=2)
    vu, vl = np.take_along_axis(up, iu[..., None], 2)[..., 0], np.take_along_axis(lw, il[..., None], 2)[..., 0]
    cu, cl = vu < s2[:, None], vl > s1[:, None]                                               # a curve is the active bound
    live &= np.where(cu, vu, s2[:, None]) > np.where(cl, vl, s1[:, None])

    def integral(idx, curve, s):
        k_, l_ = np.take_along_axis(kk, idx, 1), np.take_along_axis(lam, idx, 1)
        ta, tb = a + lc[:, None] - l_, b + lc[:, None] - l_
        return np.where(curve, np.arcsin(k_ * np.sin(tb)) - np.arcsin(k_ * np.sin(ta)), s[:, None] * (b - a))

    piece = np.where(live, integral(iu, cu, s2) - integral(il, cl, s1), 0.)
    A = np.zeros(M)
    for k in range(piece.shape[1]):                                                           # the kernel's order
        A += piece[:, k]
    return A


def overlap_areas(cube, ll, dust=DUST, device=None):
    """
    The overlap matrix in CSR form over the lat-lon cells: (row_ptr int64 [n_ll + 1], col int32 cube cells ascending within a
    row, area fp64), without the entries at or below dust * min(area_r, area_c).  device=None: this module; a HIP device: the
    kernels of csrc/overlap.hip (the result comes back to the host).
    """
    if device is not None:
        from .. import ops
        return ops.overlap_areas(cube, ll, dust, device)
    r, c = candidates(cube, ll)
    A = pair_areas(cube, ll, r, c)
    keep = A > dust * np.minimum(ll.area.ravel()[r], cube.area.ravel()[c])
    r, c, A = r[keep], c[keep], A[keep]
    row_ptr = np.zeros(ll.n_cells + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=ll.n_cells), out=row_ptr[1:])
    return row_ptr, c.astype(np.int32), A


def conservative_maps(cube, ll, device=None, dust=DUST):
    """
    The pair of first-order conservative maps between a LatLonGrid and a CubeSphereGrid as OfflineMap objects:
    (forward: lat-lon -> cube, S = A^T / cube cell area; inverse: cube -> lat-lon, S = A / lat-lon cell area).  Both carry the
    grids' dims, cell centres, areas and the covered fraction of every destination cell.
    """
    from .offline_map import OfflineMap
    row_ptr, col, A = overlap_areas(cube, ll, dust, device)
    r = np.repeat(np.arange(ll.n_cells, dtype=np.int64), np.diff(row_ptr))
    c = col.astype(np.int64)
    area_ll, area_cs = ll.area.ravel(), cube.area.ravel()
    yc_ll, xc_ll = (a.ravel() for a in np.meshgrid(ll.lat, ll.lon, indexing='ij'))
    yc_cs, xc_cs = cube.lat.ravel(), cube.lon.ravel()
    dims_ll, dims_cs = np.array([ll.n_lon, ll.n_lat], np.int32), np.array([cube.n_cells], np.int32)
    # (OfflineMap sorts the entries stably by row: handing it the columns as rows is the transpose)
    forward = OfflineMap(c + 1, r + 1, A / area_cs[c], ll.n_cells, cube.n_cells, src_grid_dims=dims_ll, dst_grid_dims=dims_cs,
                         yc_a=yc_ll, xc_a=xc_ll, yc_b=yc_cs, xc_b=xc_cs, area_a=area_ll, area_b=area_cs,
                         frac_b=np.bincount(c, A, cube.n_cells) / area_cs)
    inverse = OfflineMap(r + 1, c + 1, A / area_ll[r], cube.n_cells, ll.n_cells, src_grid_dims=dims_cs, dst_grid_dims=dims_ll,
                         yc_a=yc_cs, xc_a=xc_cs, yc_b=yc_ll, xc_b=xc_ll, area_a=area_cs, area_b=area_ll,
                         frac_b=np.bincount(r, A, ll.n_cells) / area_ll)
    return forward, inverse
