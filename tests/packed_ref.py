"""
Plain numpy restatement of the four packed-series formulas of include/dlwpcs.h (dlwpcs_channel_range, dlwpcs_pack_i16,
dlwpcs_unpack_i16, dlwpcs_batch_gather_i16) and the case tables tests/test_packed.py (CPU) and tests/test_gpu_packed.py share.

Written from the header, independent of DLWP/model/packing.py: every step is one numpy float32 operation (numpy rounds each
to nearest even, as the device does), indexing is slices and fancy indexing.  The convention: x = q * scale[v] + offset[v],
q int16 in [-32767, 32767], -32768 = missing = NaN.
"""
import numpy as np

FILL = -32768
_f = np.float32


def _col(table, ndim):
    return np.asarray(table, dtype=_f).reshape((1, -1) + (1,) * (ndim - 2))


def channel_range(x):
    """x (T, V, S) float32 -> (range (V, 2) float32 {min, max} over the finite elements, {+inf, -inf} without any;
    nonfinite (V,) int64)"""
    x = np.asarray(x, dtype=_f)
    V = x.shape[1]
    rng = np.empty((V, 2), dtype=_f)
    bad = np.empty((V,), dtype=np.int64)
    for v in range(V):
        col = x[:, v].reshape(-1)
        fin = col[np.isfinite(col)]
        rng[v] = (fin.min(), fin.max()) if fin.size else (np.inf, -np.inf)
        bad[v] = col.size - fin.size
    return rng, bad


def unclamped_codes(x, scale, offset):
    """rint((x - offset[v]) / scale[v]) as float32, before the clamp (NaN / inf where x is not finite)"""
    x = np.asarray(x, dtype=_f)
    with np.errstate(all='ignore'):
        d = x - _col(offset, x.ndim)                    # one rounded subtraction
        r = d / _col(scale, x.ndim)                     # one IEEE division
        return np.rint(r)                               # round half to even


def pack_i16(x, scale, offset):
    x = np.asarray(x, dtype=_f)
    with np.errstate(all='ignore'):
        q = np.minimum(np.maximum(unclamped_codes(x, scale, offset), _f(-32767)), _f(32767))
    q = np.where(np.isfinite(x), q, _f(FILL))
    return q.astype(np.int16)


def unpack_i16(q, scale, offset):
    q = np.asarray(q, dtype=np.int16)
    m = q.astype(_f) * _col(scale, q.ndim)              # one rounded multiplication
    r = m + _col(offset, q.ndim)                        # one rounded addition
    return np.where(q == FILL, _f(np.nan), r).astype(_f)


def bf16_bits(a):
    """bf16 bit patterns (uint16) of float32 values, rounded to nearest even; a NaN keeps its sign and top payload bits and is
    made quiet (the decoded fill code 0x7fc00000 gives 0x7fc0), as the device's conversion does.  (torch's CPU cast is not used:
    its vectorised path turns every NaN into 0xffff.)"""
    u = np.ascontiguousarray(a, dtype=_f).view(np.uint32).astype(np.uint64)
    rounded = (u + 0x7fff + ((u >> 16) & 1)) >> 16
    quiet = (u >> 16) | 0x40
    return np.where(np.isnan(a), quiet, rounded).astype(np.uint16)


def store(a, dtype):
    """round an fp32 result once to the storage type ('f32' / 'bf16'); float32 values"""
    a = np.ascontiguousarray(a, dtype=_f)
    if dtype == 'f32':
        return a
    assert dtype == 'bf16', dtype
    return (bf16_bits(a).astype(np.uint32) << 16).view(_f)


def batch_gather_i16(q, scale, offset, samples, var_idx, n_steps, t_off, t_stride, out, c_off, c_stride, channels_last, dtype):
    """writes the decoded window into a copy of `out` ((B, S, Ctot) or (B, Ctot, S)) and returns it; everything outside the
    window keeps what `out` held.  q (T, V, S) int16."""
    out = np.array(out, dtype=_f, copy=True)
    samples = np.asarray(samples, dtype=np.int64)
    var_idx = np.asarray(var_idx, dtype=np.int64)
    nv = len(var_idx)
    values = unpack_i16(q, scale, offset)
    for n in range(n_steps):
        block = store(values[samples + t_off + n * t_stride][:, var_idx, :], dtype)       # (B, nv, S)
        lo = c_off + n * c_stride
        if channels_last:
            out[:, :, lo:lo + nv] = np.transpose(block, (0, 2, 1))
        else:
            out[:, lo:lo + nv, :] = block
    return out


def bits(a):
    """the raw bit patterns of a float32 array (NaN payloads included)"""
    return np.ascontiguousarray(a, dtype=_f).view(np.uint32)


def gather_kernel(S, nv, steps, Ctot, c_off, c_stride, channels_last, array_off=0, out_off=0):
    """which form of dlwpcs_batch_gather_i16 the header says serves a call ('rows' / 'tile' / 'cf8' / 'cf1'); *_off: byte
    offset of the pointer from a 16-byte boundary"""
    wide = S % 8 == 0 and array_off % 16 == 0 and out_off % 16 == 0
    if not channels_last:
        return 'cf8' if wide else 'cf1'
    nch = nv * steps
    return 'rows' if wide and c_off == 0 and c_stride == nv and Ctot == nch and nch * 257 * 4 <= 64 * 1024 else 'tile'


# ------------------------------------------------------------------------------------------------------------------ #
# data
# ------------------------------------------------------------------------------------------------------------------ #

def families(rng, T=6, S=97):
    """name -> (T, V, S) float32: the data families the round-trip bound is checked on"""
    n = lambda *s: rng.standard_normal(s)                                                   # noqa: E731
    out = {}
    out['unit'] = (n(T, 4, S) + np.array([0.0, 3.0, -250.0, 1e4])[None, :, None]).astype(_f)
    out['geopotential'] = (4.5e4 + (5.9e4 - 4.5e4) * rng.random((T, 2, S))).astype(_f)
    out['pressure'] = (101325.0 + 1e-3 * n(T, 2, S)).astype(_f)          # a range below fp32 resolution at this magnitude
    spans = 10.0 ** np.arange(-6, 7, 2)
    out['ranges'] = (n(T, len(spans), S) * spans[None, :, None]).astype(_f)
    out['constant'] = np.broadcast_to(np.array([0.0, -7.25, 101325.0, 1e-30], dtype=_f)[None, :, None], (T, 4, S)).copy()
    return out


def special_array(rng, T, V, S):
    """(T, V, S) float32: variable 0 ordinary data with NaN, +inf and -inf sprinkled in, the last variable all NaN, and (V >= 3)
    variable 1 constant"""
    x = (rng.standard_normal((T, V, S)) * 3.0 + 1.5).astype(_f)
    x[0, 0, 0], x[T // 2, 0, 5], x[T - 1, 0, S - 1] = np.nan, np.inf, -np.inf
    x[:, V - 1] = np.nan
    if V >= 3:
        x[:, 1] = _f(-7.25)
    return x


def gather_codes(rng, T, V, S):
    """int16 codes with both ends of the range and the fill code present in every variable"""
    q = rng.integers(-32767, 32768, size=(T, V, S), dtype=np.int64).astype(np.int16)
    q[:, :, 0] = 32767
    q[:, :, 1] = -32767
    q[:, :, S // 2] = FILL
    q[T // 2, :, S - 1] = FILL
    return q


def gather_tables(rng, V):
    """scale (one negative) and offset per variable"""
    scale = (10.0 ** rng.uniform(-4, 1, V)).astype(_f)
    scale[V // 2] = -scale[V // 2]
    offset = (rng.standard_normal(V) * 100.0).astype(_f)
    return scale, offset


# dlwpcs_batch_gather_i16 cases: T = 7, B = 3 (a repeated sample), V = nv + 2, a permuted var_idx; steps == 2: t_stride 2, t_off 1.
# win = (Ctot, c_off, c_stride) or None for "the gathered channels are the whole row".
_G = [
    # dt,    kern,   S,   nv, steps, win,        cl
    ('f32',  'tile', 150, 3, 2, None,        True),       # a partial last 64-pixel tile
    ('bf16', 'tile', 150, 1, 1, None,        True),
    ('f32',  'rows', 384, 3, 2, None,        True),       # one full and one half 256-pixel tile
    ('bf16', 'rows', 384, 3, 2, None,        True),
    ('f32',  'rows', 384, 1, 1, None,        True),
    ('bf16', 'rows', 384, 1, 1, None,        True),       # an odd channel count with bf16 output
    ('bf16', 'rows', 384, 3, 1, None,        True),
    ('f32',  'tile', 388, 3, 2, None,        True),       # S % 8 != 0 falls back
    ('bf16', 'tile', 388, 3, 2, None,        True),
    ('f32',  'tile', 384, 3, 2, (11, 2, 4),  True),       # a window inside a wider row: c_off > 0, Ctot > n_steps * nv
    ('bf16', 'tile', 384, 1, 2, (5, 1, 2),   True),
    ('f32',  'cf8',  384, 3, 2, None,        False),
    ('bf16', 'cf8',  384, 3, 2, (11, 2, 4),  False),
    ('f32',  'cf1',  150, 3, 2, (11, 2, 4),  False),
    ('bf16', 'cf1',  388, 1, 1, None,        False),
    ('f32',  'cf1',  388, 3, 1, None,        False),
]
GATHER = [dict(dt=d, kern=k, S=S, nv=nv, steps=st, win=w, cl=cl) for d, k, S, nv, st, w, cl in _G]
GATHER_T, GATHER_B = 7, 3
GATHER_SAMPLES = np.array([2, 0, 2], dtype=np.int32)


def gather_geometry(case):
    """(Ctot, c_off, c_stride, t_off, t_stride) of a GATHER case"""
    nch = case['nv'] * case['steps']
    Ctot, c_off, c_stride = case['win'] if case['win'] else (nch, 0, case['nv'])
    t_off, t_stride = (1, 2) if case['steps'] > 1 else (2, 1)
    return Ctot, c_off, c_stride, t_off, t_stride


# generator configurations shared by the CPU and the GPU tests: name -> ArrayDataGenerator keywords (_sol / _const: feed the
# insolation array / the constants)
GENERATORS = {
    'single': dict(rank=3, batch_size=3, input_time_steps=2, output_time_steps=2, channels_last=True),
    'sequence': dict(rank=3, batch_size=4, input_slice=slice(0, 3), output_slice=slice(1, 4), input_time_steps=2,
                     output_time_steps=2, sequence=2, channels_last=True, _sol=True, _const=True),
    'interval2': dict(rank=3, batch_size=4, input_time_steps=2, output_time_steps=1, interval=2, channels_last=True, _sol=True),
    'channels_first': dict(rank=3, batch_size=5, input_slice=[3, 0, 2], output_slice=[1, 3], input_time_steps=1,
                           output_time_steps=1, channels_last=False, _const=True),
}


def generator_data(seed=5, T=20, V=4, N=4):
    """(array (T, V, 6, N, N), insolation (T, 6, N, N), constants (2, 6, N, N)), float32"""
    rng = np.random.default_rng(seed)
    arr = (rng.standard_normal((T, V, 6, N, N)) * np.array([1.0, 30.0, 0.02, 5.0])[:V].reshape(1, V, 1, 1, 1)
           + np.array([0.0, 5e4, 1.0, -3.0])[:V].reshape(1, V, 1, 1, 1)).astype(_f)
    sol = rng.random((T, 6, N, N)).astype(_f)
    const = rng.standard_normal((2, 6, N, N)).astype(_f)
    return arr, sol, const


class Meta(object):
    """the model metadata an ArrayDataGenerator reads"""
    is_convolutional, is_recurrent, impute = True, False, False


def make_generator(name, array, sol, const, **extra):
    from DLWP.model.generators import ArrayDataGenerator
    kw = dict(GENERATORS[name])
    use_sol, use_const = kw.pop('_sol', False), kw.pop('_const', False)
    kw.update(extra)
    return ArrayDataGenerator(Meta(), array, insolation_array=sol if use_sol else None, constants=const if use_const else None,
                              **kw)
