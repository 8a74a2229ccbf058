"""
A small reader of netCDF classic files (CDF-1) and 64-bit-offset files (CDF-2), and a writer of the latter, after the public
"NetCDF Classic and 64-bit Offset Format" specification: big-endian header of dimensions, global attributes and variables,
then the data of the fixed-size variables and the interleaved records.  numpy is the only dependency.  netCDF-4 (HDF5) and
CDF-5 files are not read; the writer makes fixed-size variables only (no record dimension).
"""
import os

import numpy as np

NC_DIMENSION, NC_VARIABLE, NC_ATTRIBUTE = 0x0A, 0x0B, 0x0C
_TYPES = {1: np.dtype('>i1'), 2: np.dtype('S1'), 3: np.dtype('>i2'), 4: np.dtype('>i4'), 5: np.dtype('>f4'), 6: np.dtype('>f8')}


class _Header(object):
    def __init__(self, buf, name):
        self.buf, self.pos, self.name = buf, 0, name

    def take(self, n):
        if self.pos + n > len(self.buf):
            raise ValueError('%s: truncated netCDF header (needs %d bytes at offset %d, file has %d)'
                             % (self.name, n, self.pos, len(self.buf)))
        out = self.buf[self.pos:self.pos + n]
        self.pos += n
        return out

    def u32(self):
        return int(np.frombuffer(self.take(4), '>u4')[0])

    def u64(self):
        return int(np.frombuffer(self.take(8), '>u8')[0])

    def string(self):
        n = self.u32()
        s = self.take(n)
        self.take((-n) % 4)
        return s.decode('utf-8', 'replace')

    def values(self):
        t = self.u32()
        if t not in _TYPES:
            raise ValueError('%s: unknown netCDF type %d in an attribute' % (self.name, t))
        n = self.u32()
        nb = n * _TYPES[t].itemsize
        raw = self.take(nb)
        self.take((-nb) % 4)
        if t == 2:
            return raw.decode('utf-8', 'replace')
        return np.frombuffer(raw, _TYPES[t]).astype(_TYPES[t].newbyteorder('='))

    def tagged_list(self, tag):
        t, n = self.u32(), self.u32()
        if t == 0 and n == 0:
            return 0
        if t != tag:
            raise ValueError('%s: malformed netCDF header (tag 0x%x where 0x%x was expected)' % (self.name, t, tag))
        return n

    def attributes(self):
        return {self.string(): self.values() for _ in range(self.tagged_list(NC_ATTRIBUTE))}


class NetCDFClassic(object):
    """
    A parsed classic / 64-bit-offset netCDF file.  `dims` {name: length} (the record dimension: the number of records),
    `attrs` the global attributes, `variables` {name: (dims, dtype, attrs)}; `read(name)` returns a variable's values as a
    native-endian numpy array.  Raises ValueError for a file that is not one, or is shorter than its header says.
    """

    def __init__(self, path):
        self.path = path
        with open(path, 'rb') as f:
            self._buf = f.read()
        name = os.path.basename(path)
        h = _Header(self._buf, name)
        magic = h.take(4)
        if magic[:3] != b'CDF' or magic[3] not in (1, 2):
            if magic[:3] == b'CDF' and magic[3] == 5:
                raise ValueError('%s: CDF-5 (64-bit data) netCDF files are not read' % name)
            raise ValueError('%s: not a netCDF classic or 64-bit-offset file' % name)
        self.version = magic[3]
        numrecs = h.u32()
        self.numrecs = 0 if numrecs == 0xFFFFFFFF else numrecs     # streaming: counted from the file size below
        streaming = numrecs == 0xFFFFFFFF
        self._dim_names, self._dim_lens = [], []
        self.record_dim = None
        for _ in range(h.tagged_list(NC_DIMENSION)):
            dn, dl = h.string(), h.u32()
            if dl == 0:
                self.record_dim = len(self._dim_names)
            self._dim_names.append(dn)
            self._dim_lens.append(dl)
        self.attrs = h.attributes()
        self._vars = {}
        order = []
        for _ in range(h.tagged_list(NC_VARIABLE)):
            vn = h.string()
            ids = [h.u32() for _ in range(h.u32())]
            if any(i >= len(self._dim_names) for i in ids):
                raise ValueError('%s: variable %r names a dimension that does not exist' % (name, vn))
            va = h.attributes()
            t = h.u32()
            if t not in _TYPES:
                raise ValueError('%s: variable %r has unknown netCDF type %d' % (name, vn, t))
            vsize = h.u32()
            begin = h.u32() if self.version == 1 else h.u64()
            self._vars[vn] = (ids, _TYPES[t], va, vsize, begin)
            order.append(vn)
        rec = [v for v in order if self._is_record(self._vars[v][0])]
        self._recsize = 0
        for v in rec:
            ids, dt, _, vsize, _ = self._vars[v]
            n = int(np.prod([self._dim_lens[i] for i in ids[1:]], dtype=np.int64)) * dt.itemsize
            self._recsize += n if len(rec) == 1 else n + (-n) % 4
        if streaming and rec and self._recsize:
            first = min(self._vars[v][4] for v in rec)
            self.numrecs = max(0, (len(self._buf) - first) // self._recsize)
        self.dims = {d: (self.numrecs if i == self.record_dim else n)
                     for i, (d, n) in enumerate(zip(self._dim_names, self._dim_lens))}
        self.variables = {v: (tuple(self._dim_names[i] for i in ids), dt.newbyteorder('='), va)
                          for v, (ids, dt, va, _, _) in self._vars.items()}
        for v in order:                                           # every variable's data must lie inside the file
            self._extent(v)

    def _is_record(self, ids):
        return bool(ids) and ids[0] == self.record_dim

    def _shape(self, ids):
        return tuple(self.numrecs if i == self.record_dim else self._dim_lens[i] for i in ids)

    def _extent(self, v):
        ids, dt, _, _, begin = self._vars[v]
        shape = self._shape(ids)
        if self._is_record(ids):
            per = int(np.prod(shape[1:], dtype=np.int64)) * dt.itemsize
            end = begin + (shape[0] - 1) * self._recsize + per if shape[0] else begin
        else:
            end = begin + int(np.prod(shape, dtype=np.int64)) * dt.itemsize
        if end > len(self._buf):
            raise ValueError('%s: truncated file: variable %r ends at byte %d, the file has %d'
                             % (os.path.basename(self.path), v, end, len(self._buf)))
        return shape, dt, begin

    def __contains__(self, v):
        return v in self._vars

    def read(self, v):
        if v not in self._vars:
            raise KeyError(v)
        shape, dt, begin = self._extent(v)
        if not self._is_record(self._vars[v][0]):
            n = int(np.prod(shape, dtype=np.int64))
            out = np.frombuffer(self._buf, dt, count=n, offset=begin).reshape(shape)
        else:
            per = int(np.prod(shape[1:], dtype=np.int64))
            out = np.empty(shape, dt)
            for r in range(shape[0]):
                out[r] = np.frombuffer(self._buf, dt, count=per, offset=begin + r * self._recsize).reshape(shape[1:])
        if dt == np.dtype('S1'):
            return out.copy()
        return out.astype(dt.newbyteorder('='))


_TYPE_IDS = {np.dtype(dt.str[1:]): t for t, dt in _TYPES.items() if t != 2}


def _pad4(b):
    return b + b'\0' * ((-len(b)) % 4)


def _name(s):
    b = s.encode('utf-8')
    return np.array(len(b), '>u4').tobytes() + _pad4(b)


def _attributes(attrs):
    if not attrs:
        return np.zeros(2, '>u4').tobytes()
    out = np.array([NC_ATTRIBUTE, len(attrs)], '>u4').tobytes()
    for k, v in attrs.items():
        if isinstance(v, str):
            raw, t, n = v.encode('utf-8'), 2, len(v.encode('utf-8'))
        else:
            a = np.atleast_1d(np.asarray(v))
            if a.dtype not in _TYPE_IDS:
                a = a.astype(np.int32 if np.issubdtype(a.dtype, np.integer) else np.float64)
            raw, t, n = a.astype(_TYPES[_TYPE_IDS[a.dtype]]).tobytes(), _TYPE_IDS[a.dtype], a.size
        out += _name(k) + np.array([t, n], '>u4').tobytes() + _pad4(raw)
    return out


def write_netcdf(path, dims, variables, attrs=None):
    """
    Write a 64-bit-offset (CDF-2) netCDF file of fixed-size variables.

    :param dims: {name: length}, every length positive (a zero length would declare the record dimension)
    :param variables: iterable of (name, dim names, array) or (name, dim names, array, attributes); int8 / int16 / int32 /
        float32 / float64 arrays are stored as they are, other integers as int32 (checked) and other floats as float64
    :param attrs: global attributes {name: str or numbers}
    """
    names = list(dims)
    for d, n in dims.items():
        if int(n) < 1 or int(n) >= 2 ** 31:
            raise ValueError('dimension %s = %r: a fixed dimension has 1 .. 2^31 - 1 entries' % (d, n))
    head = b'CDF\x02' + np.zeros(1, '>u4').tobytes()
    head += np.array([NC_DIMENSION, len(names)], '>u4').tobytes() if names else np.zeros(2, '>u4').tobytes()
    for d in names:
        head += _name(d) + np.array(int(dims[d]), '>u4').tobytes()
    head += _attributes(attrs)
    entries = []
    for var in variables:
        vn, vd, arr = var[0], tuple(var[1]), np.asarray(var[2])
        va = var[3] if len(var) > 3 else None
        if arr.dtype not in _TYPE_IDS:
            if np.issubdtype(arr.dtype, np.integer):
                if arr.size and (arr.min() < -2 ** 31 or arr.max() >= 2 ** 31):
                    raise ValueError('variable %s does not fit int32' % vn)
                arr = arr.astype(np.int32)
            else:
                arr = arr.astype(np.float64)
        shape = tuple(int(dims[d]) for d in vd)
        if arr.size != int(np.prod(shape, dtype=np.int64)):
            raise ValueError('variable %s has %d values, its dimensions %s hold %s' % (vn, arr.size, vd, shape))
        t = _TYPE_IDS[arr.dtype]
        raw = _pad4(np.ascontiguousarray(arr).astype(_TYPES[t]).tobytes())
        if len(raw) >= 2 ** 32:
            raise ValueError('variable %s is too large for the 64-bit-offset format' % vn)
        meta = _name(vn) + np.array([len(vd)] + [names.index(d) for d in vd], '>u4').tobytes() + _attributes(va) + \
            np.array([t, len(raw)], '>u4').tobytes()
        entries.append((meta, raw))
    head += np.array([NC_VARIABLE, len(entries)], '>u4').tobytes() if entries else np.zeros(2, '>u4').tobytes()
    begin = len(head) + sum(len(m) + 8 for m, _ in entries)
    with open(path, 'wb') as f:
        body = b''
        for meta, raw in entries:
            body += meta + np.array(begin, '>u8').tobytes()
            begin += len(raw)
        f.write(head + body)
        for _, raw in entries:
            f.write(raw)
