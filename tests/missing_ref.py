"""
Plain-loop reference of the masked application of an offline map (include/dlwpcs.h, dlwpcs_sparse_map_apply_masked) and the
maps, fields and bounds tests/test_remap_missing.py (CPU) and tests/test_gpu_remap_missing.py share.  Not a test module.

Written from the header: one destination row and one position at a time, the row's CSR entries in order.  The DECISION (which
outputs are missing) is taken in np.float32 arithmetic, one rounded operation per step, as the kernel takes it; the VALUES are
fp64 sums, as DLWP.remap.OfflineMap.apply_host keeps them.
"""
import functools

import numpy as np

import remap_maps as rm

_f = np.float32
MIN_VALID = (0.0, 0.3, 0.5, 1.0)


def apply_masked(m, x, min_valid, renormalize):
    """x (n_a, Q) float -> (y (n_b, Q) float64 with NaN where missing, frac (n_b, Q) float32)"""
    x = np.asarray(x)
    Q = x.shape[1]
    y = np.zeros((m.n_b, Q), dtype=np.float64)
    frac = np.zeros((m.n_b, Q), dtype=_f)
    mv = _f(min_valid)
    for r in range(m.n_b):
        for q in range(Q):
            acc = wval64 = wall64 = 0.0
            wval, wall = _f(0), _f(0)
            nval = nmiss = 0
            for j in range(int(m.row_ptr[r]), int(m.row_ptr[r + 1])):
                v = m.val[j]
                if v == 0:
                    continue                                    # neither present nor missing
                wall = _f(wall + v)
                wall64 += m.val64[j]
                a = x[m.col[j], q]
                if np.isnan(a):
                    nmiss += 1
                else:
                    acc += m.val64[j] * float(a)
                    wval = _f(wval + v)
                    wval64 += m.val64[j]
                    nval += 1
            if nmiss > 0 and (wval < _f(mv * wall) or nval == 0 or mv >= _f(1)):
                y[r, q] = np.nan
            elif renormalize and nmiss > 0:
                y[r, q] = acc * (wall64 / wval64)
            else:
                y[r, q] = acc
            frac[r, q] = _f(wval / wall) if nval + nmiss > 0 else _f(0)
    return y, frac


def apply_plain(m, x, axes):
    """OfflineMap.apply_host without missing values, restated: fp64 sums slot by slot, the input's float dtype back"""
    x = np.asarray(x)
    a0, a1 = m._space(x.shape, axes)
    pre, post = x.shape[:a0], x.shape[a1:]
    P, Q = int(np.prod(pre, dtype=np.int64)), int(np.prod(post, dtype=np.int64))
    xs = x.reshape(P, m.n_a, Q)
    y = np.zeros((P, m.n_b, Q), dtype=np.float64)
    lengths = np.diff(m.row_ptr.astype(np.int64))
    for s in range(int(lengths.max()) if lengths.size else 0):
        rows = np.nonzero(lengths > s)[0]
        j = m.row_ptr[rows].astype(np.int64) + s
        y[:, rows, :] += m.val64[j][None, :, None] * xs[:, m.col[j], :].astype(np.float64)
    dt = x.dtype if np.issubdtype(x.dtype, np.floating) else np.float64
    return y.reshape(pre + tuple(m.dst_shape) + post).astype(dt, copy=False)


def nonneg(m):
    """the entries of m with |weight| (skipna serves weights >= 0 only), the destination a plain list of n_b cells"""
    from DLWP.remap import OfflineMap
    rows = np.repeat(np.arange(m.n_b, dtype=np.int64), np.diff(m.row_ptr.astype(np.int64)))
    return OfflineMap(rows + 1, m.col.astype(np.int64) + 1, np.abs(m.val64), m.n_a, m.n_b, dst_cells=True)


@functools.lru_cache(maxsize=None)
def maps():
    """name -> OfflineMap: the maps of the issue.  'random' has empty rows, duplicates and unsorted entries; 'bilinear1' (triangle
    rows only: a cube of one cell per face) and 'bilinear2' carry entries of weight exactly 0."""
    from DLWP.remap import CubeSphereGrid, LatLonGrid, bilinear_map, conservative_maps
    out = {'small': rm.cube_to_latlon(8, 12, 24, s=2)}
    out['cons13_fwd'], out['cons13_inv'] = conservative_maps(CubeSphereGrid(8), LatLonGrid.cells(13, 24))
    out['cons19_fwd'], out['cons19_inv'] = conservative_maps(CubeSphereGrid(8), LatLonGrid.cells(19, 36))
    out['random'] = nonneg(rm.random_map(np.random.default_rng(5), 50, 300, 700, empty_rows=60, duplicates=11))
    rng = np.random.default_rng(11)
    for N in (1, 2):
        out['bilinear%d' % N] = bilinear_map(CubeSphereGrid(N), rng.uniform(-90, 90, 150), rng.uniform(0, 360, 150))
    assert int(np.diff(out['cons19_fwd'].row_ptr).max()) == 18
    assert (np.diff(out['random'].row_ptr) == 0).any()
    assert (out['bilinear1'].val == 0).sum() == 150 and (out['bilinear2'].val == 0).any()
    return out


UNIT_ROWS = ('small', 'cons13_fwd', 'cons13_inv', 'cons19_fwd', 'cons19_inv', 'bilinear1', 'bilinear2')   # rows that sum to 1


def field(m, rng, lead=(), trail=(), holes=0.2):
    """random float32 field lead + src_shape + trail with the share `holes` of its elements NaN"""
    x = rng.standard_normal(tuple(lead) + tuple(m.src_shape) + tuple(trail)).astype(_f)
    if holes:
        x[rng.random(x.shape) < holes] = np.nan
    return x


def row_weights(m):
    """(n_max: the longest row's entries, max_r wall_r in fp64)"""
    lengths = np.diff(m.row_ptr.astype(np.int64))
    rows = np.repeat(np.arange(m.n_b), lengths)
    wall = np.bincount(rows, np.abs(m.val64), minlength=m.n_b)
    return int(lengths.max()), float(wall.max())


def value_bar(m, x):
    """(2 n_max + 3) 2^-24 max|x| max_r wall_r: n_max fma roundings of partial sums that never exceed max|x| wall_r, the two
    fp32 weight sums behind the renormalisation factor, one division and one multiplication"""
    n_max, wall = row_weights(m)
    ax = np.abs(x)[~np.isnan(x)]
    return (2 * n_max + 3) * 2.0 ** -24 * (float(ax.max()) if ax.size else 0.0) * wall      # (a field of nothing but holes: 0)


def ulp_distance(a, b):
    """|a - b| in units in the last place of float32 values of one sign (here: fractions in [0, 1])"""
    ia = np.ascontiguousarray(a, dtype=_f).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b, dtype=_f).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)
