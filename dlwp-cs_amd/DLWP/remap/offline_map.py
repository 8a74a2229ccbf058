"""
Offline remapping maps (the SCRIP / TempestRemap layout written by GenerateOfflineMap): a sparse matrix S of n_b x n_a with
entries (row, col, S), 1-based, plus the shapes and cell centres of the two grids.  `OfflineMap` validates the entries, sorts
them into CSR form and applies the matrix to stacks of fields: on the host in fp64 (numpy inputs), or on a HIP device with
the dlwpcs_sparse_map_apply kernel (device tensors).
"""
import os

import numpy as np

from ..labelled import is_tensor as _is_tensor
from .netcdf_classic import NetCDFClassic, write_netcdf

_REQUIRED = ('row', 'col', 'S')
_NETCDF4_MSG = ('%s is a netCDF-4 (HDF5) file, which is not read; convert it to the 64-bit-offset format with '
                '`nccopy -k 64-bit-offset in.nc out.nc`, or regenerate it with CubeSphereRemap(to_netcdf4=False)')


def _cube_side(n):
    if n % 6:
        return None
    s = int(round(np.sqrt(n // 6)))
    return s if 6 * s * s == n and s > 0 else None


def _constant_along(a, axis):
    return bool(np.all(a == np.take(a, [0], axis=axis)))


class _Grid(object):
    """shape of one side of a map, its kind ('cube', 'latlon' or 'cells'), 1-D lat / lon for a lat-lon grid, and the
    permutation (file cell index of each cell in `shape` order, or None) that puts a lon-major file into (lat, lon) order"""

    def __init__(self, n, dims, yc, xc, side, cells=False):
        self.order = None
        self.lat = self.lon = None
        dims = None if dims is None else [int(d) for d in np.ravel(dims)]
        if dims is not None and int(np.prod(dims, dtype=np.int64)) != n:
            raise ValueError('%s_grid_dims %s do not multiply to n_%s = %d' % (side, dims, 'a' if side == 'src' else 'b', n))
        if dims is None or len(dims) == 1:
            s = None if cells else _cube_side(n)
            self.kind, self.shape = ('cube', (6, s, s)) if s else ('cells', (n,))
        elif len(dims) == 2:
            self.kind = 'latlon'
            fast, slow = dims                                    # SCRIP order: the fastest-varying axis first
            if yc is None or xc is None:
                self.shape = (slow, fast)                        # (lat, lon) as the dims say; nothing to check against
            else:
                y, x = np.asarray(yc, np.float64).reshape(slow, fast), np.asarray(xc, np.float64).reshape(slow, fast)
                if _constant_along(y, 1) and _constant_along(x, 0):
                    self.shape = (slow, fast)
                    self.lat, self.lon = y[:, 0].copy(), x[0, :].copy()
                elif _constant_along(y, 0) and _constant_along(x, 1):
                    # lon-major file: the latitude varies fastest.  Cell (i_lat, i_lon) is file cell i_lon * n_lat + i_lat.
                    self.shape = (fast, slow)
                    self.order = np.arange(n, dtype=np.int64).reshape(slow, fast).T.ravel()
                    self.lat, self.lon = y[0, :].copy(), x[:, 0].copy()
                else:
                    raise ValueError('%s grid: yc / xc are neither lat-major nor lon-major on its %s grid dims (the '
                                     'latitude must be constant along the longitude)' % (side, dims))
        else:
            raise ValueError('%s grid of rank %d is not served (rank 1: cubed sphere or cells, rank 2: lat-lon)'
                             % (side, len(dims)))


class OfflineMap(object):
    """
    A remapping matrix of n_b destination cells x n_a source cells.

    :param row, col: 1-based destination / source cell of every entry (as in the file)
    :param S: weight of every entry
    :param n_a, n_b: source and destination cell counts
    :param src_grid_dims, dst_grid_dims: SCRIP grid dims (fastest axis first): rank 1 of 6 N^2 cells is a cubed sphere
        (6, N, N) in face-major order; rank 2 is a lat-lon grid, whose orientation is checked against yc / xc
    :param yc_a, xc_a, yc_b, xc_b: cell-centre latitudes / longitudes in degrees (optional)
    :param area_a, area_b, frac_b: cell areas in steradians of the two grids and the covered fraction of every destination
        cell (optional; carried, not used by `apply`)
    :param dst_cells: a rank-1 destination is a list of n_b cells or points ('cells') even when n_b is 6 N^2

    Entries are sorted stably by row into CSR (`row_ptr` int32 [n_b + 1], `col` int32 0-based, `val` fp32, `val64` fp64);
    duplicate (row, col) pairs stay separate terms, empty rows are allowed.  Raises ValueError for entries that do not fit.
    """

    def __init__(self, row, col, S, n_a, n_b, src_grid_dims=None, dst_grid_dims=None, yc_a=None, xc_a=None, yc_b=None,
                 xc_b=None, name=None, area_a=None, area_b=None, frac_b=None, dst_cells=False):
        self.name = name
        self.n_a, self.n_b = int(n_a), int(n_b)
        if self.n_a < 0 or self.n_b < 0:
            raise ValueError('n_a = %d and n_b = %d must not be negative' % (self.n_a, self.n_b))
        row, col, S = np.ravel(row), np.ravel(col), np.ravel(S)
        if not (row.shape == col.shape == S.shape):
            raise ValueError('row, col and S have different lengths (%d, %d, %d)' % (row.size, col.size, S.size))
        for a, nm in ((row, 'row'), (col, 'col')):
            if a.size and not np.issubdtype(a.dtype, np.integer):
                if not np.all(np.isfinite(a)) or not np.all(a == np.round(a)):
                    raise ValueError('%s holds non-integer indices' % nm)
        row, col = row.astype(np.int64), col.astype(np.int64)
        S = np.asarray(S, dtype=np.float64)
        if row.size >= 2 ** 31:
            raise ValueError('%d entries: at most 2^31 - 1 are served' % row.size)
        if row.size and (row.min() < 1 or row.max() > self.n_b):
            raise ValueError('row indices must lie in [1, n_b = %d]; found %d .. %d' % (self.n_b, row.min(), row.max()))
        if col.size and (col.min() < 1 or col.max() > self.n_a):
            raise ValueError('col indices must lie in [1, n_a = %d]; found %d .. %d' % (self.n_a, col.min(), col.max()))
        if not np.all(np.isfinite(S)):
            raise ValueError('S holds %d non-finite weights' % int((~np.isfinite(S)).sum()))
        src = _Grid(self.n_a, src_grid_dims, yc_a, xc_a, 'src')
        dst = _Grid(self.n_b, dst_grid_dims, yc_b, xc_b, 'dst', cells=bool(dst_cells))
        row0, col0 = row - 1, col - 1
        if src.order is not None:
            col0 = np.argsort(src.order)[col0]
        if dst.order is not None:
            row0 = np.argsort(dst.order)[row0]
        self.src_shape, self.dst_shape = src.shape, dst.shape
        self._dst_order = dst.order
        self.src_kind, self.dst_kind = src.kind, dst.kind
        self.lat_a, self.lon_a, self.lat_b, self.lon_b = src.lat, src.lon, dst.lat, dst.lon
        self.yc_a, self.xc_a = self._ordered(yc_a, src.order), self._ordered(xc_a, src.order)
        self.yc_b, self.xc_b = self._ordered(yc_b, dst.order), self._ordered(xc_b, dst.order)
        self.area_a, self.area_b = self._ordered(area_a, src.order), self._ordered(area_b, dst.order)
        self.frac_b = self._ordered(frac_b, dst.order)
        for a, n, nm in ((self.area_a, self.n_a, 'area_a'), (self.area_b, self.n_b, 'area_b'), (self.frac_b, self.n_b, 'frac_b')):
            if a is not None and a.size != n:
                raise ValueError('%s has %d entries for %d cells' % (nm, a.size, n))
        order = np.argsort(row0, kind='stable')
        self.row_ptr = np.zeros(self.n_b + 1, dtype=np.int32)
        np.cumsum(np.bincount(row0, minlength=self.n_b), out=self.row_ptr[1:])
        self.col = col0[order].astype(np.int32)
        self.val64 = S[order]
        self.val = self.val64.astype(np.float32)
        self.nnz = int(self.col.size)
        self._device = {}

    @staticmethod
    def _ordered(c, order):
        if c is None:
            return None
        c = np.asarray(c, dtype=np.float64).ravel()
        return c if order is None else c[order]

    def __repr__(self):
        return 'OfflineMap(%s%s -> %s, %d entries)' % ('%s: ' % self.name if self.name else '', self.src_shape, self.dst_shape,
                                                      self.nnz)

    # ---------------------------------------------------------------------------------------------------------------- #
    def to(self, device):
        """(row_ptr, col, val) as device tensors, uploaded once per device and kept.  Raises NativeError when the first
        upload to a device would happen inside a graph capture."""
        import torch
        from .._native import NativeError
        key = str(torch.device(device))
        hit = self._device.get(key)
        if hit is None:
            if torch.cuda.is_current_stream_capturing():
                raise NativeError('the remapping map would have to be uploaded during graph capture; apply it once eagerly '
                                  'first')
            hit = tuple(torch.from_numpy(a).to(device) for a in (self.row_ptr, self.col, self.val))
            self._device[key] = hit
        return hit

    def _space(self, shape, axes):
        nd = len(shape)
        ax = sorted(int(a) % nd for a in (axes if hasattr(axes, '__len__') else (axes,)))
        if len(set(ax)) != len(ax) or ax != list(range(ax[0], ax[0] + len(ax))):
            raise ValueError('space axes %s must be distinct and consecutive' % (tuple(axes),))
        got = tuple(int(s) for s in shape[ax[0]:ax[-1] + 1])
        if got != tuple(self.src_shape) and got != (self.n_a,):
            raise ValueError('space axes %s have shape %s; the map reads %s' % (tuple(axes), got, self.src_shape))
        return ax[0], ax[-1] + 1

    def check_skipna(self, min_valid):
        """what skipna=True asks of the map and of min_valid (ValueError otherwise): no negative weight -- the share of a row's
        weight that is present must grow with every present entry -- and 0 <= min_valid <= 1"""
        if not (0.0 <= float(min_valid) <= 1.0):
            raise ValueError('min_valid = %r must lie in [0, 1]' % (min_valid,))
        neg = getattr(self, '_has_negative', None)
        if neg is None:
            neg = self._has_negative = bool(self.val.size and self.val.min() < 0)
        if neg:
            raise ValueError('%s holds negative weights: skipna=True serves maps with weights >= 0 only' % self)

    def apply(self, x, axes, out=None, skipna=False, min_valid=0.5, renormalize=True, frac_out=None):
        """
        Apply the map to the source grid held in the consecutive `axes` of x; they are replaced by the destination grid
        (dst_shape).  numpy input: the host path (fp64 sums, the input's float dtype back).  HIP tensor: one
        dlwpcs_sparse_map_apply launch on the current stream, fp32 result (`out`: a float32 tensor or view to write to).

        skipna=True: NaN in x is a missing value (see `apply_host`; on the device dlwpcs_sparse_map_apply_masked).  frac_out:
        True, or on the device a float32 tensor to write to: the present share of every output's weight is returned too, as
        (y, frac).
        """
        if isinstance(x, np.ndarray) or not _is_tensor(x):
            if out is not None:
                raise ValueError('out= is for device tensors')
            if frac_out is not None and frac_out is not True and frac_out is not False:
                raise ValueError('frac_out= a tensor is for device tensors; frac_out=True returns it')
            return self.apply_host(np.asarray(x), axes, skipna=skipna, min_valid=min_valid, renormalize=renormalize,
                                   frac_out=frac_out)
        from .. import ops
        return ops.sparse_map_apply(self, x, axes, out=out, skipna=skipna, min_valid=min_valid, renormalize=renormalize,
                                    frac_out=frac_out)

    def apply_host(self, x, axes, skipna=False, min_valid=0.5, renormalize=True, frac_out=None):
        """
        numpy restatement of the kernel with fp64 accumulation; float inputs keep their dtype, others give float64.

        skipna=True restates dlwpcs_sparse_map_apply_masked (include/dlwpcs.h): a NaN in x is missing, an entry whose fp32 weight
        is 0 is not there.  Which outputs are missing is decided exactly as the kernel decides it -- `wval` and `wall`, the fp32
        sums in CSR order of the fp32 weights of the present / of all entries; missing iff an entry is missing and
        (wval < float32(min_valid) * wall, or none is present, or min_valid >= 1) -- so host and device agree on every NaN.
        The values keep fp64: the sum over the present entries, times (all weight / present weight) in fp64 with `renormalize`.
        frac_out=True: (y, frac) with frac = wval / wall in float32 (1 where nothing is missing, 0 for a row without entries).
        """
        x = np.asarray(x)
        if not skipna:
            if frac_out is not None and frac_out is not False:
                raise ValueError('frac_out needs skipna=True')
            return self._apply_host_plain(x, axes)
        self.check_skipna(min_valid)
        a0, a1 = self._space(x.shape, axes)
        pre, post = x.shape[:a0], x.shape[a1:]
        P, Q = int(np.prod(pre, dtype=np.int64)), int(np.prod(post, dtype=np.int64))
        xs = x.reshape(P, self.n_a, Q)
        f32 = np.float32
        acc = np.zeros((P, self.n_b, Q), dtype=np.float64)
        wval64 = np.zeros((P, self.n_b, Q), dtype=np.float64)
        wall64 = np.zeros(self.n_b, dtype=np.float64)
        wval = np.zeros((P, self.n_b, Q), dtype=f32)
        wall = np.zeros(self.n_b, dtype=f32)
        nval = np.zeros((P, self.n_b, Q), dtype=np.int32)
        nmiss = np.zeros((P, self.n_b, Q), dtype=np.int32)
        lengths = np.diff(self.row_ptr.astype(np.int64))
        for s in range(int(lengths.max()) if lengths.size else 0):
            rows = np.nonzero(lengths > s)[0]
            j = self.row_ptr[rows].astype(np.int64) + s
            there = self.val[j] != 0                            # decided on the fp32 weight, as on the device
            rows, j = rows[there], j[there]
            if not rows.size:
                continue
            xv = xs[:, self.col[j], :].astype(np.float64)
            ok = ~np.isnan(xv)
            v32, v64 = self.val[j][None, :, None], self.val64[j][None, :, None]
            acc[:, rows, :] += np.where(ok, v64 * np.where(ok, xv, 0.0), 0.0)
            wval64[:, rows, :] += np.where(ok, v64, 0.0)
            wall64[rows] += self.val64[j]
            wval[:, rows, :] = wval[:, rows, :] + np.where(ok, v32, f32(0))       # one rounded fp32 addition per entry
            wall[rows] = wall[rows] + self.val[j]
            nval[:, rows, :] += ok
            nmiss[:, rows, :] += ~ok
        need = (f32(min_valid) * wall)[None, :, None]           # one rounded fp32 multiplication
        holes = nmiss > 0
        missing = holes & ((wval < need) | (nval == 0) | (f32(min_valid) >= f32(1)))
        y = acc
        with np.errstate(all='ignore'):
            if renormalize:
                y = np.where(holes, acc * (wall64[None, :, None] / wval64), acc)
            y = np.where(missing, np.nan, y)
            frac = np.where((nval + nmiss) > 0, wval / wall[None, :, None], f32(0)).astype(f32)
        dt = x.dtype if np.issubdtype(x.dtype, np.floating) else np.float64
        shape = pre + tuple(self.dst_shape) + post
        y = y.reshape(shape).astype(dt, copy=False)
        return (y, frac.reshape(shape)) if frac_out else y

    def _apply_host_plain(self, x, axes):
        a0, a1 = self._space(x.shape, axes)
        pre, post = x.shape[:a0], x.shape[a1:]
        P, Q = int(np.prod(pre, dtype=np.int64)), int(np.prod(post, dtype=np.int64))
        xs = x.reshape(P, self.n_a, Q)
        y = np.zeros((P, self.n_b, Q), dtype=np.float64)
        lengths = np.diff(self.row_ptr.astype(np.int64))
        for s in range(int(lengths.max()) if lengths.size else 0):
            rows = np.nonzero(lengths > s)[0]
            j = self.row_ptr[rows].astype(np.int64) + s
            y[:, rows, :] += self.val64[j][None, :, None] * xs[:, self.col[j], :].astype(np.float64)
        dt = x.dtype if np.issubdtype(x.dtype, np.floating) else np.float64
        return y.reshape(pre + tuple(self.dst_shape) + post).astype(dt, copy=False)

    def masked(self, mask, min_valid=0.5, renormalize=True):
        """
        (map, frac): this map with a FIXED mask over its source cells (True / non-zero = missing, shape self.src_shape or
        (n_a,)) folded into the weights once, on the host: the entries of masked cells are dropped, the others scaled by
        (all weight / present weight) of their row in fp64 with `renormalize`, and a row that `apply(..., skipna=True,
        min_valid=min_valid)` would give as NaN for a field with NaN at the mask -- the same fp32 decision -- becomes EMPTY.
        The plain kernel then serves a fixed land-sea mask at no cost per call: the new map applied to a field with any
        finite value at the masked cells gives what the dynamic form gives with NaN there, and 0 where that gives NaN.
        frac: float32 of self.dst_shape, the present share of every row's weight (1 for an untouched row, 0 for a row without
        entries); rows with 0 < frac and no entries left are the dropped ones.
        """
        self.check_skipna(min_valid)
        mask = np.asarray(mask).astype(bool).reshape(-1)
        if mask.size != self.n_a:
            raise ValueError('mask has %d cells; the map reads %d' % (mask.size, self.n_a))
        f32 = np.float32
        rows = np.repeat(np.arange(self.n_b, dtype=np.int64), np.diff(self.row_ptr.astype(np.int64)))
        there = self.val != 0
        ok = there & ~mask[self.col]
        wall, wval = np.zeros(self.n_b, dtype=f32), np.zeros(self.n_b, dtype=f32)
        wall64, wval64 = np.zeros(self.n_b, dtype=np.float64), np.zeros(self.n_b, dtype=np.float64)
        start = self.row_ptr[:-1].astype(np.int64)
        lengths = np.diff(self.row_ptr.astype(np.int64))
        for s in range(int(lengths.max()) if lengths.size else 0):
            r = np.nonzero(lengths > s)[0]
            j = start[r] + s
            wall[r] = wall[r] + np.where(there[j], self.val[j], f32(0))
            wval[r] = wval[r] + np.where(ok[j], self.val[j], f32(0))
            wall64[r] += np.where(there[j], self.val64[j], 0.0)
            wval64[r] += np.where(ok[j], self.val64[j], 0.0)
        nval = np.bincount(rows[ok], minlength=self.n_b)
        nmiss = np.bincount(rows[there & ~ok], minlength=self.n_b)
        holes = nmiss > 0
        dropped = holes & ((wval < f32(min_valid) * wall) | (nval == 0) | (f32(min_valid) >= f32(1)))
        with np.errstate(all='ignore'):
            frac = np.where((nval + nmiss) > 0, wval / wall, f32(0)).astype(f32)
            factor = np.where(holes & ~dropped, wall64 / wval64, 1.0) if renormalize else np.ones(self.n_b)
        keep = ok & ~dropped[rows]
        out = OfflineMap(rows[keep] + 1, self.col[keep].astype(np.int64) + 1, self.val64[keep] * factor[rows[keep]], self.n_a, self.n_b,
                         name=self.name, dst_cells=self.dst_kind == 'cells')
        # the grids as this map holds them (already in (lat, lon) / face order: nothing to re-derive from file conventions)
        for a in ('src_shape', 'dst_shape', '_dst_order', 'src_kind', 'dst_kind', 'lat_a', 'lon_a', 'lat_b', 'lon_b', 'yc_a', 'xc_a',
                  'yc_b', 'xc_b', 'area_a', 'area_b'):
            setattr(out, a, getattr(self, a))
        out.frac_b = frac.astype(np.float64)
        return out, frac.reshape(self.dst_shape)


def read_offline_map(path):
    """
    Read an offline map file (netCDF classic or 64-bit offset) into an OfflineMap.  Raises FileNotFoundError for a missing
    file and ValueError for a netCDF-4 file, a file of another format, a truncated file, a missing variable or entries that
    do not fit the grids.
    """
    if not os.path.exists(path):
        raise FileNotFoundError(path)
    from ..keras.hdf5_lite import is_hdf5
    if is_hdf5(path):
        raise ValueError(_NETCDF4_MSG % path)
    nc = NetCDFClassic(path)
    missing = [v for v in _REQUIRED if v not in nc]
    if missing:
        raise ValueError('%s: required variable(s) %s missing' % (path, ', '.join(missing)))
    for d in ('n_a', 'n_b'):
        if d not in nc.dims:
            raise ValueError('%s: required dimension %s missing' % (path, d))
    opt = {v: (nc.read(v) if v in nc else None) for v in ('src_grid_dims', 'dst_grid_dims', 'yc_a', 'xc_a', 'yc_b', 'xc_b',
                                                          'area_a', 'area_b', 'frac_b')}
    return OfflineMap(nc.read('row'), nc.read('col'), nc.read('S'), nc.dims['n_a'], nc.dims['n_b'],
                      name=os.path.basename(path), **opt)


def _scrip_dims(kind, shape):
    return [int(shape[1]), int(shape[0])] if kind == 'latlon' else [int(np.prod(shape, dtype=np.int64))]


def write_offline_map(m, path):
    """
    Write an OfflineMap as a 64-bit-offset netCDF file in the SCRIP layout that read_offline_map reads: n_a, n_b, n_s, row, col
    (1-based), S (fp64), the grid dims (fastest axis first; a lat-lon grid is written lat-major, as the map holds it) and
    whichever of yc_* / xc_* / area_* / frac_b the map carries.
    """
    if m.nnz < 1 or m.n_a < 1 or m.n_b < 1:
        raise ValueError('%s has no entries or no cells: nothing to write' % m)
    src, dst = _scrip_dims(m.src_kind, m.src_shape), _scrip_dims(m.dst_kind, m.dst_shape)
    dims = {'n_a': m.n_a, 'n_b': m.n_b, 'n_s': m.nnz, 'src_grid_rank': len(src), 'dst_grid_rank': len(dst)}
    row = np.repeat(np.arange(1, m.n_b + 1, dtype=np.int32), np.diff(m.row_ptr.astype(np.int64)))
    variables = [('src_grid_dims', ('src_grid_rank',), np.array(src, np.int32)),
                 ('dst_grid_dims', ('dst_grid_rank',), np.array(dst, np.int32))]
    for nm, units in (('yc', 'degrees'), ('xc', 'degrees'), ('area', 'steradians')):
        for side in 'ab':
            a = getattr(m, '%s_%s' % (nm, side), None)
            if a is not None:
                variables.append(('%s_%s' % (nm, side), ('n_%s' % side,), a, {'units': units}))
    if getattr(m, 'frac_b', None) is not None:
        variables.append(('frac_b', ('n_b',), m.frac_b))
    variables += [('row', ('n_s',), row), ('col', ('n_s',), m.col.astype(np.int32) + 1), ('S', ('n_s',), m.val64)]
    write_netcdf(path, dims, variables, attrs={'title': 'first-order conservative offline map', 'normalization': 'destarea'})
