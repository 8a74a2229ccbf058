"""
The training series as 16-bit codes: `PackedSeries` holds a (time, variable, *space) array as int16 plus two floats per
variable, in the CF / netCDF packing convention ERA5 itself is distributed in,

    x = q * scale_factor[v] + add_offset[v],    q in [-32767, 32767],    -32768 = missing = NaN.

Half the bytes of the fp32 array, in HBM as on the host: the device-resident `ArrayDataGenerator` uploads the codes as they
are and its gathers decode on the way (`dlwpcs_batch_gather_i16`), so a series twice as long stays resident and the gathers
read half as much.  After per-variable scaling a variable spans a few standard deviations; 65 532 codes over that range
resolve about 1e-4 of one, far below what bf16 activations see.

Every arithmetic step, on the host (numpy float32) and on the device, is one rounded fp32 operation -- subtract, IEEE divide,
round half to even, clamp on the way in; multiply, add on the way out -- so host and device give the same codes and the same
decoded bits, and a generator's host path over a `PackedSeries` is the bit pattern of its device path.

A `PackedSeries` looks like the array it stands for where the generator and the estimator need it to: `.shape`, `len()`,
indexing of the leading axis (decoded fp32 numpy rows) and `np.asarray`.
"""
import numpy as np

FILL = -32768
CODES = 65532                # the linear codes spread over [lo, hi]: +-32766 around the mid-range
_HOST_ROWS_BYTES = 1 << 28   # host packing / decoding works through the time axis in blocks of about this many fp32 bytes
_DEVICE_ROWS_BYTES = 1 << 30


def _is_tensor(x):
    return hasattr(x, 'is_cuda') and hasattr(x, 'data_ptr')


def _bc(table, ndim):
    """a (V,) table shaped to broadcast against (rows, V, *space)"""
    return table.reshape((1, -1) + (1,) * (ndim - 2))


def encode(x, scale, offset):
    """int16 codes of the float32 array x (rows, V, *space): subtract, divide, rint, clamp; NaN / inf -> -32768"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all='ignore'):
        d = x - _bc(offset, x.ndim)
        r = d / _bc(scale, x.ndim)
        q = np.clip(np.rint(r), np.float32(-32767), np.float32(32767))
        return np.where(np.isfinite(x), q, np.float32(FILL)).astype(np.int16)


def decode(q, scale, offset):
    """float32 values of the int16 codes q (rows, V, *space): multiply, add; -32768 -> NaN"""
    q = np.asarray(q)
    m = q.astype(np.float32) * _bc(scale, q.ndim)
    r = m + _bc(offset, q.ndim)
    r[q == FILL] = np.nan
    return r


def tables_from_range(lo, hi):
    """
    (scale_factor, add_offset), float32 (V,), from the per-variable {min, max} over the finite values (float32; an empty
    range is lo = +inf, hi = -inf).  Formed in float64 and rounded once:
        scale = max((hi - lo) / 65532, 2^-22 * max(|lo|, |hi|)),    offset = (hi + lo) / 2.
    The floor keeps a code no finer than float32 resolves at the variable's magnitude (a nearly constant field), so the
    clamp at +-32767 never bites.  A variable without a finite value, or whose scale comes out 0 (all zeros), gets scale 1.
    """
    lo = np.asarray(lo, dtype=np.float32).astype(np.float64).reshape(-1)
    hi = np.asarray(hi, dtype=np.float32).astype(np.float64).reshape(-1)
    some = lo <= hi
    lo, hi = np.where(some, lo, 0.0), np.where(some, hi, 0.0)
    scale = np.maximum((hi - lo) / CODES, 2.0 ** -22 * np.maximum(np.abs(lo), np.abs(hi))).astype(np.float32)
    offset = ((hi + lo) / 2.0 + 0.0).astype(np.float32)          # (+ 0.0: a range of signed zeros gives +0 either way)
    scale[scale == 0] = 1.0
    return scale, offset


def _time_blocks(shape, block_bytes):
    T = int(shape[0])
    row = 4 * int(np.prod(shape[1:], dtype=np.int64)) if len(shape) > 1 else 4
    step = max(1, int(block_bytes // max(row, 1)))
    return [(a, min(a + step, T)) for a in range(0, T, step)]


def host_range(array):
    """per-variable (lo, hi) over the finite float32 values of array (T, V, *space); (+inf, -inf) where there are none"""
    V = int(array.shape[1])
    lo, hi = np.full(V, np.inf, dtype=np.float32), np.full(V, -np.inf, dtype=np.float32)
    for a, b in _time_blocks(array.shape, _HOST_ROWS_BYTES):
        x = np.moveaxis(np.asarray(array[a:b], dtype=np.float32), 1, 0).reshape(V, -1)
        fin = np.isfinite(x)
        lo = np.minimum(lo, np.where(fin, x, np.float32(np.inf)).min(axis=1, initial=np.float32(np.inf)))
        hi = np.maximum(hi, np.where(fin, x, np.float32(-np.inf)).max(axis=1, initial=np.float32(-np.inf)))
    return lo, hi


class PackedSeries(object):
    """
    A (time, variable, *space) series held as int16 codes `q` with per-variable `scale_factor` / `add_offset` (see the module
    docstring).  `q` lives on the host (numpy) or on a device (torch tensor); `scale_factor` and `add_offset` are float32
    numpy arrays either way, `scale` / `offset` are the same tables beside the codes (device tensors for device codes), which
    is what `DLWP.ops.batch_gather` reads.
    """

    def __init__(self, q, scale_factor, add_offset):
        """
        Wrap codes that already exist (ERA5's own int16 variables stacked along the variable axis, say).
        :param q: int16 numpy array or device tensor (time, variable, *space)
        :param scale_factor, add_offset: one value per variable; every scale non-zero (negative is legal)
        """
        if _is_tensor(q):
            import torch
            if q.dtype != torch.int16:
                raise TypeError('PackedSeries: codes must be int16, got %s' % q.dtype)
            q = q.contiguous()
        else:
            q = np.asarray(q)
            if q.dtype != np.int16:
                raise TypeError('PackedSeries: codes must be int16, got %s' % q.dtype)
        if q.ndim < 2:
            raise ValueError('PackedSeries: codes must be (time, variable, *space), got shape %s' % (tuple(q.shape),))
        V = int(q.shape[1])
        scale = np.array(scale_factor, dtype=np.float32).reshape(-1)
        offset = np.array(add_offset, dtype=np.float32).reshape(-1)
        if scale.size != V or offset.size != V:
            raise ValueError('PackedSeries: %d scale factors and %d offsets for %d variables' % (scale.size, offset.size, V))
        if not np.all(np.isfinite(scale)) or np.any(scale == 0) or not np.all(np.isfinite(offset)):
            raise ValueError('PackedSeries: every scale factor must be finite and non-zero, every offset finite')
        self.q = q
        self.scale_factor, self.add_offset = scale, offset
        if _is_tensor(q):
            import torch
            self.scale, self.offset = torch.from_numpy(scale).to(q.device), torch.from_numpy(offset).to(q.device)
        else:
            self.scale, self.offset = scale, offset

    # ------------------------------------------------------------------------------------------------------------- #
    @classmethod
    def pack(cls, array, device=None):
        """
        Pack a float array (time, variable, *space): the per-variable range of its finite values gives the tables
        (`tables_from_range`), non-finite elements become the fill code.  device=None and a host array: packed with numpy,
        the series stays on the host.  A device (or an fp32 device tensor as `array`): the ranges come from
        `dlwpcs_channel_range`, the codes from `dlwpcs_pack_i16`, and the series is device-resident; a host array goes up in
        blocks of rows, so the fp32 form never has to fit beside the codes.  Both ways give the same codes and tables.
        """
        if _is_tensor(array):
            return cls._pack_device(array, array.device if device is None else device)
        if not hasattr(array, 'shape') or not hasattr(array, '__getitem__'):
            array = np.asarray(array, dtype=np.float32)
        if len(array.shape) < 2:
            raise ValueError('PackedSeries.pack: expected (time, variable, *space), got shape %s' % (tuple(array.shape),))
        if device is not None and device is not False:
            return cls._pack_device(array, device)
        scale, offset = tables_from_range(*host_range(array))
        q = np.empty(tuple(array.shape), dtype=np.int16)
        for a, b in _time_blocks(array.shape, _HOST_ROWS_BYTES):
            q[a:b] = encode(array[a:b], scale, offset)
        return cls(q, scale, offset)

    @classmethod
    def _pack_device(cls, array, device):
        import torch
        from .. import ops
        from ..keras import backend
        dev = backend.device() if device is True else torch.device(device)
        if _is_tensor(array):
            blocks = [(0, int(array.shape[0]))]
            block = lambda a, b: array.to(device=dev, dtype=torch.float32).contiguous()        # noqa: E731
        else:
            blocks = _time_blocks(array.shape, _DEVICE_ROWS_BYTES)
            block = lambda a, b: torch.from_numpy(np.ascontiguousarray(array[a:b], dtype=np.float32)).to(dev)   # noqa: E731
        V = int(array.shape[1])
        lo, hi = np.full(V, np.inf, dtype=np.float32), np.full(V, -np.inf, dtype=np.float32)
        x = None
        for a, b in blocks:
            x = block(a, b)
            rng = ops.channel_range(x)[0].cpu().numpy()
            lo, hi = np.minimum(lo, rng[:, 0]), np.maximum(hi, rng[:, 1])
        scale, offset = tables_from_range(lo, hi)
        sd, od = torch.from_numpy(scale).to(dev), torch.from_numpy(offset).to(dev)
        q = torch.empty(tuple(array.shape), dtype=torch.int16, device=dev)
        for a, b in blocks:
            if len(blocks) > 1 or x is None:
                x = block(a, b)
            ops.pack_i16(x, sd, od, out=q[a:b])
        return cls(q, scale, offset)

    # ------------------------------------------------------------------------------------------------------------- #
    @property
    def device(self):
        """the device of the codes; None for a host series"""
        return self.q.device if _is_tensor(self.q) else None

    @property
    def shape(self):
        return tuple(int(s) for s in self.q.shape)

    @property
    def ndim(self):
        return len(self.q.shape)

    @property
    def dtype(self):
        """the dtype of what indexing returns"""
        return np.dtype(np.float32)

    @property
    def nbytes(self):
        """the bytes this series occupies: the codes and the two tables"""
        return 2 * int(np.prod(self.shape, dtype=np.int64)) + 8 * self.shape[1]

    def __len__(self):
        return self.shape[0]

    def to_device(self, device):
        """this series with its codes on `device` (itself when they already are)"""
        import torch
        from ..keras import backend
        dev = backend.device() if device is True else torch.device(device)
        if _is_tensor(self.q):
            if self.q.device == dev or (dev.index is None and self.q.device.type == dev.type):
                return self
            return PackedSeries(self.q.to(dev), self.scale_factor, self.add_offset)
        return PackedSeries(torch.from_numpy(np.ascontiguousarray(self.q)).to(dev), self.scale_factor, self.add_offset)

    def has_fill(self):
        """is any element the missing-value code?"""
        if _is_tensor(self.q):
            return bool((self.q == FILL).any().item())
        return bool((self.q == FILL).any())

    def missing_counts(self):
        """(time, variable) int32: the number of missing-value codes of every plane -- numpy for host codes, a device tensor
        from one dlwpcs_missing_count pass for device codes"""
        from .. import ops
        if _is_tensor(self.q):
            return ops.missing_counts(self)
        return ops.missing_counts_host(self.q)

    # ------------------------------------------------------------------------------------------------------------- #
    def _decode_rows(self, q, variables=None):
        """decoded fp32 of a block of code rows (n, V, *space), optionally of the listed variables only: numpy for host codes,
        a device tensor for device codes"""
        if _is_tensor(q):
            import torch
            from .. import ops
            scale, offset = self.scale, self.offset
            if variables is not None:
                sel = torch.from_numpy(np.asarray(variables, dtype=np.int64)).to(q.device)
                q, scale, offset = q.index_select(1, sel), scale[sel].contiguous(), offset[sel].contiguous()
            return ops.unpack_i16(q.contiguous(), scale, offset)
        if variables is not None:
            v = np.asarray(variables, dtype=np.int64)
            return decode(q[:, v], self.scale_factor[v], self.add_offset[v])
        return decode(q, self.scale_factor, self.add_offset)

    def __getitem__(self, index):
        """rows of the leading axis -- an int, a slice or an integer index array -- decoded: float32 numpy"""
        if isinstance(index, tuple):
            raise IndexError('PackedSeries: only the leading (time) axis can be indexed; decode with unpack() for more')
        single = isinstance(index, (int, np.integer))
        if _is_tensor(self.q):
            import torch
            if single:
                rows = self.q[int(index)].unsqueeze(0)
            elif isinstance(index, slice):
                rows = self.q[index]
            else:
                idx = np.asarray(index)
                if idx.dtype == bool or idx.ndim != 1:
                    raise IndexError('PackedSeries: index arrays are one-dimensional integers')
                idx = idx.astype(np.int64)
                n = self.shape[0]
                if idx.size and (idx.min() < -n or idx.max() >= n):
                    raise IndexError('index %d is out of bounds for axis 0 with size %d'
                                     % (int(idx.max() if idx.max() >= n else idx.min()), n))
                rows = self.q.index_select(0, torch.from_numpy(np.where(idx < 0, idx + n, idx)).to(self.q.device))
            out = self._decode_rows(rows).cpu().numpy()
        else:
            if single:
                rows = self.q[int(index)][np.newaxis]
            elif isinstance(index, slice):
                rows = self.q[index]
            else:
                idx = np.asarray(index)
                if idx.dtype == bool or idx.ndim != 1:
                    raise IndexError('PackedSeries: index arrays are one-dimensional integers')
                rows = self.q[idx.astype(np.int64)]
            out = self._decode_rows(rows)
        return out[0] if single else out

    def unpack(self, variables=None):
        """
        The whole series decoded to float32 (time, variable, *space), or only the listed variables of it: a numpy array for
        host codes, a device tensor for device codes.
        """
        if _is_tensor(self.q):
            return self._decode_rows(self.q, variables)
        nv = self.shape[1] if variables is None else len(np.asarray(variables).reshape(-1))
        out = np.empty((self.shape[0], nv) + self.shape[2:], dtype=np.float32)
        for a, b in _time_blocks(out.shape, _HOST_ROWS_BYTES):
            out[a:b] = self._decode_rows(self.q[a:b], variables)
        return out

    def __array__(self, dtype=None, copy=None):
        x = self.unpack()
        if _is_tensor(x):
            x = x.cpu().numpy()
        return x if dtype is None else x.astype(dtype, copy=False)

    def __repr__(self):
        where = 'host' if self.device is None else str(self.device)
        return 'PackedSeries(shape=%s, %s, %d bytes)' % (self.shape, where, self.nbytes)
