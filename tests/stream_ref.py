"""
Plain numpy references of the streaming helper operations of libdlwpcs (include/dlwpcs.h: padding layer, activation, 2x2
pooling / upsampling and their adjoints, concat / split, channel pad / slice, rollout state repack, layout converters, add,
batch gather), written from the header's doc comments and the Keras layer semantics: indexing is reshape / repeat / slices /
fancy indexing, never a flattened-offset formula.

Conventions
  * tensors are numpy arrays in the shapes the header documents; a bf16 tensor is a float32 array whose values are bf16 values
    (every bf16 value is an fp32 value), or, for pure data movement, any array -- the movers only index;
  * arithmetic operations evaluate the documented fp32 expression in np.float32 and round ONCE to the storage type
    (`store`: torch's CPU cast, round-to-nearest-even, for 'bf16'; nothing for 'f32');
  * `vec_*`: the documented rule by which a host entry point picks its storage vector (csrc/elementwise.hip, dispatch_vec /
    dispatch_mover / the flat kernels), restated so that a test can name the kernel instantiation a case is there for.

tests/test_stream_ref.py checks these references against the fp64 oracle (oracle/cs_oracle.py) on the CPU;
tests/test_gpu_stream_ops.py compares the device kernels with them bit for bit.
"""
import numpy as np
import torch

F32, BF16 = 'f32', 'bf16'
_f = np.float32


# ------------------------------------------------------------------------------------------------------------------ #
# storage
# ------------------------------------------------------------------------------------------------------------------ #

def store(a, dtype):
    """round an fp32 result once to the storage type; returns float32 values"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if dtype == F32:
        return a
    assert dtype == BF16, dtype
    return torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy()


def bf16_ulp(v):
    """spacing of bf16 at |v| (8 significant bits)"""
    v = abs(float(v))
    if v == 0.0 or not np.isfinite(v):
        return 2.0 ** -133
    return 2.0 ** (int(np.floor(np.log2(v))) - 7)


def bf16_floor(v):
    """largest bf16 <= v (v >= 0)"""
    u = np.array([v], dtype=np.float32).view(np.uint32) & np.uint32(0xffff0000)
    return float(u.view(np.float32)[0])


# ------------------------------------------------------------------------------------------------------------------ #
# which storage vector serves a call (the documented dispatch rules)
# ------------------------------------------------------------------------------------------------------------------ #

def esize(dtype):
    return 2 if dtype == BF16 else 4


def vec_arith(dtype, *counts):
    """arithmetic kernels: the widest vector (8 / 2 / 1 bf16, 4 / 1 fp32 channels) dividing every channel count in play"""
    if dtype == BF16:
        if all(c % 8 == 0 for c in counts):
            return 'H8'
        return 'H2' if all(c % 2 == 0 for c in counts) else 'bf16'
    return 'float4' if all(c % 4 == 0 for c in counts) else 'float'


def vec_mover(dtype, *counts):
    """pure data movement: the widest of 16 / 4 / 2 bytes dividing the byte length of every channel run"""
    b = [c * esize(dtype) for c in counts]
    if all(x % 16 == 0 for x in b):
        return 'u128'
    return 'u32' if all(x % 4 == 0 for x in b) else 'u16'


def vec_flat(dtype, *byte_offsets):
    """flat kernels (activation, add): 16-B vectors plus a scalar tail when every pointer is 16-B aligned, else scalars"""
    ok = all(o % 16 == 0 for o in byte_offsets)
    if dtype == BF16:
        return 'H8' if ok else 'bf16'
    return 'float4' if ok else 'float'


def vec_word(dtype):
    """kernels that move raw elements one by one (state repack, channel pad / slice, layout converters)"""
    return 'u16' if dtype == BF16 else 'u32'


def vec_width(vec):
    return {'H8': 8, 'H2': 2, 'bf16': 1, 'float4': 4, 'float': 1}[vec]


def mover_items(dtype, vec, n_elements):
    """work items of a mover launch that writes n_elements elements"""
    return n_elements * esize(dtype) // {'u128': 16, 'u32': 4, 'u16': 2}[vec]


def gather_kernel(dtype, S, nv, n_steps, Ctot, c_off, c_stride, channels_last, aligned=True):
    """which batch-gather kernel serves a call: 'rows' (256-pixel tiles, whole output rows written as 16-B vectors), 'tile'
    (64-pixel LDS tiles) or 'cf' (channels_first)"""
    if not channels_last:
        return 'cf'
    nch = nv * n_steps
    whole_rows = c_off == 0 and c_stride == nv and Ctot == nch
    even = nch % 2 == 0 if dtype == BF16 else True
    fits = nch * 257 * 4 <= 64 * 1024
    return 'rows' if (whole_rows and S % 4 == 0 and even and fits and aligned) else 'tile'


# ------------------------------------------------------------------------------------------------------------------ #
# padding layer
# ------------------------------------------------------------------------------------------------------------------ #

def inverse_table(table, N, p):
    """(6*N*N, 4) int32 from a halo table (6, M, M): for every source cell the padded cells outside the face interior that read
    it, in ascending order of their flat index, -1 in the unused slots (dlwpcs_halo_inverse_table)."""
    M = N + 2 * p
    table = np.asarray(table).reshape(6, M, M)
    inv = np.full((6 * N * N, 4), -1, dtype=np.int32)
    cnt = np.zeros(6 * N * N, dtype=np.int64)
    halo = np.ones((6, M, M), dtype=bool)
    halo[:, p:p + N, p:p + N] = False
    for dst in np.flatnonzero(halo.reshape(-1)):
        src = int(table.reshape(-1)[dst])
        inv[src, cnt[src]] = dst
        cnt[src] += 1
    return inv


def pad_fwd(x, table):
    """y (B,6,M,M,C): every padded cell is a copy of the source cell the table names"""
    B, C = x.shape[0], x.shape[-1]
    M = table.shape[-1]
    return x.reshape(B, -1, C)[:, np.asarray(table).reshape(-1).astype(np.int64)].reshape(B, 6, M, M, C)


def pad_bwd(dy, N, p, inv, dtype):
    """dx[src] = dy[own copy of src] + the extra padded cells of the inverse table, added one slot after the other in fp32"""
    dy = np.asarray(dy, dtype=np.float32)
    B, C = dy.shape[0], dy.shape[-1]
    acc = dy[:, :, p:p + N, p:p + N, :].reshape(B, 6 * N * N, C).copy()
    flat = dy.reshape(B, -1, C)
    inv = np.asarray(inv).reshape(6 * N * N, 4)
    for k in range(4):
        cells = np.flatnonzero(inv[:, k] >= 0)
        acc[:, cells] = acc[:, cells] + flat[:, inv[cells, k].astype(np.int64)]
    return store(acc.reshape(B, 6, N, N, C), dtype)


# ------------------------------------------------------------------------------------------------------------------ #
# keras ReLU(negative_slope = alpha, max_value = vmax)
# ------------------------------------------------------------------------------------------------------------------ #

def act_fwd(x, alpha, vmax, dtype):
    """min(x, vmax) for x >= 0, alpha * x for x < 0 (NaN stays NaN)"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        y = np.where(x >= 0, np.minimum(x, _f(vmax)), _f(alpha) * x)
    return store(y.astype(np.float32), dtype)


def act_slope(x, alpha, vmax):
    """derivative of the activation at the PRE-activation x: alpha below 0, 1 inside (0, vmax), 0 elsewhere"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        return np.where(x < 0, _f(alpha), np.where((x > 0) & (x < _f(vmax)), _f(1), _f(0))).astype(np.float32)


def act_bwd(dy, x, alpha, vmax, dtype):
    """dx = dy * act'(x), one rounding"""
    return store(np.asarray(dy, dtype=np.float32) * act_slope(x, alpha, vmax), dtype)


# ------------------------------------------------------------------------------------------------------------------ #
# AveragePooling3D((1,2,2)) / UpSampling3D((1,2,2)), channels_last (B,6,N,N,C)
# ------------------------------------------------------------------------------------------------------------------ #

def _quads(x):
    x = np.asarray(x, dtype=np.float32)
    return x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 0::2], x[:, :, 1::2, 1::2]


def _spread(a):
    return np.repeat(np.repeat(a, 2, axis=2), 2, axis=3)


def avgpool2_fwd(x, dtype):
    a, b, c, d = _quads(x)
    return store(((a + b) + (c + d)) * _f(0.25), dtype)


def avgpool2_bwd(dy, dtype):
    return store(_spread(np.asarray(dy, dtype=np.float32)) * _f(0.25), dtype)


def avgpool2_bwd_add(dy, dskip, dtype):
    return store(np.asarray(dskip, dtype=np.float32) + _spread(np.asarray(dy, dtype=np.float32)) * _f(0.25), dtype)


def avgpool2_bwd_masked(dy, dskip, slope, dtype):
    """(dskip + 0.25 dy spread) * act'(m); `slope` = act' of the pooled tensor's own activation (act_slope), dskip may be None"""
    g = _spread(np.asarray(dy, dtype=np.float32)) * _f(0.25)
    if dskip is not None:
        g = np.asarray(dskip, dtype=np.float32) + g
    return store(g * np.asarray(slope, dtype=np.float32), dtype)


def upsample2_fwd(x):
    return _spread(x)


def upsample2_bwd(dy, dtype):
    a, b, c, d = _quads(dy)
    return store((a + b) + (c + d), dtype)


# ------------------------------------------------------------------------------------------------------------------ #
# channel movers, add
# ------------------------------------------------------------------------------------------------------------------ #

def concat2(a, b):
    return np.concatenate([a, b], axis=-1)


def split2(y, Ca):
    return y[..., :Ca].copy(), y[..., Ca:].copy()


def pad_channels(x, Cp):
    y = np.zeros(x.shape[:-1] + (Cp,), dtype=x.dtype)
    y[..., :x.shape[-1]] = x
    return y


def slice_channels(y, C):
    return y[..., :C].copy()


def state_repack(state, extra, T):
    """state (B,S,T*V), extra (B,T,S,E) -> (B,S,T*(V+E)): extra's channels behind the V state channels of every time step"""
    B, S = state.shape[:2]
    st = state.reshape(B, S, T, -1)
    ex = np.transpose(extra, (0, 2, 1, 3))
    return np.concatenate([st, ex], axis=-1).reshape(B, S, -1)


def cf_to_cl(x):
    return np.ascontiguousarray(np.transpose(x, (0, 2, 1)))


def cl_to_cf(x):
    return np.ascontiguousarray(np.transpose(x, (0, 2, 1)))


def add(a, b, dtype):
    return store(np.asarray(a, dtype=np.float32) + np.asarray(b, dtype=np.float32), dtype)


# ------------------------------------------------------------------------------------------------------------------ #
# batch gather
# ------------------------------------------------------------------------------------------------------------------ #

def batch_gather(array, samples, var_idx, n_steps, t_off, t_stride, out, c_off, c_stride, channels_last, dtype):
    """writes the gathered window into a copy of `out` ((B,S,Ctot) or (B,Ctot,S)) and returns it; everything outside the
    window keeps what `out` held.  array (T,V,S) fp32."""
    out = np.array(out, dtype=np.float32, copy=True)
    samples = np.asarray(samples, dtype=np.int64)
    var_idx = np.asarray(var_idx, dtype=np.int64)
    nv = len(var_idx)
    for n in range(n_steps):
        block = store(array[samples + t_off + n * t_stride][:, var_idx, :], dtype)        # (B, nv, S)
        lo = c_off + n * c_stride
        if channels_last:
            out[:, :, lo:lo + nv] = np.transpose(block, (0, 2, 1))
        else:
            out[:, lo:lo + nv, :] = block
    return out
