"""
GPU tests of the per-variable scaling kernels (dlwp-cs_amd/csrc/scaling.hip: dlwpcs_channel_moments, dlwpcs_channel_affine), their
ops wrappers and DLWP.model.preprocessing on device tensors.  References: tests/scaling_ref.py (numpy).  Moments are held to the
a-priori fp64 reordering bound with exact counts, the affine to the bits of numpy's float32 arithmetic.
"""
import ctypes

import numpy as np
import pytest
import torch

import scaling_ref as sr

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
U = 2.0 ** -24


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _desc(R, C, S, src, dst=(0, 0, 0)):
    from DLWP import _native as nat
    d = nat.ChanDesc()
    d.R, d.C, d.S = R, C, S
    d.row_stride, d.chan_stride, d.inner_stride = src
    d.dst_row_stride, d.dst_chan_stride, d.dst_inner_stride = dst
    return d


def _abi_moments(mem, R, C, S, strides, rows=None, center=None, skipna=False):
    """dlwpcs_channel_moments on the device buffer `mem` read through (R, C, S, strides) -> (C, 3) numpy"""
    from DLWP import _native as nat
    lib = nat.lib()
    d = _desc(R, C, S, strides)
    rows_d = None if rows is None else _dev(np.asarray(rows, dtype=np.int32))
    n_rows = 0 if rows is None else int(rows_d.numel())
    ctr = None if center is None else _dev(np.asarray(center, dtype=np.float64))
    out = torch.full((C, 3), -7.0, dtype=torch.float64, device=DEV)
    nbytes = int(lib.dlwpcs_channel_moments_scratch_bytes(ctypes.byref(d), n_rows))
    scratch = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=DEV)
    nat.check(lib.dlwpcs_channel_moments(ctypes.byref(d), mem.data_ptr(), nat.ptr(rows_d), n_rows, nat.ptr(ctr), int(skipna),
                                         out.data_ptr(), scratch.data_ptr(), nbytes, nat.stream_ptr()), 'dlwpcs_channel_moments')
    return out.cpu().numpy()


def _check_moments(got, x, rows, center, skipna, what):
    """x: the logical (R, C, S) array.  Counts exact; a NaN sum where the reference's is NaN; otherwise within the bound."""
    want = sr.moments(x, rows, center, skipna)
    bound = sr.moments_bound(x, rows, center)
    assert got.shape == want.shape and got.dtype == np.float64, what
    assert np.array_equal(got[:, 0], want[:, 0]), (what, got[:, 0], want[:, 0])
    for k in (1, 2):
        nan = np.isnan(want[:, k])
        assert np.array_equal(np.isnan(got[:, k]), nan), (what, k, got[:, k], want[:, k])
        err = np.abs(got[~nan, k] - want[~nan, k])
        assert np.all(err <= bound[~nan, k]), (what, k, err, bound[~nan, k])


def _data(R, C, S, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((R, C, S)) * (1. + np.arange(C))[None, :, None] + 10. * np.arange(C)[None, :, None] - 5.
    return x.astype(np.float32)


def _with_nans(x):
    """NaN in the first and the last element of a row, and in one whole row"""
    x = x.copy()
    R, C, S = x.shape
    x[0, 0, 0] = np.nan
    x[R // 2, C - 1, S - 1] = np.nan
    x[R - 1, C // 2, :] = np.nan
    return x


def _row_lists(R):
    out = [None]
    if R >= 2:
        out.append(np.arange(0, R, 2))                                              # a strided subset
        out.append(np.array([R - 1, 0, R // 2, 0] + list(range(R - 1, 0, -3))))     # unsorted, with a duplicate
    return out


# rows: 1, 2, around the unroll of 8 rows, around a slab of 8 rows (slabs are whole multiples of the unroll: 16 rows are two
# slabs, 17 three), 37 = several workgroups per channel
ROWS = (1, 2, 7, 8, 9, 15, 16, 17, 37)


@pytest.mark.parametrize('S', [96, 1024, 1028, 1030, 97])
def test_moments_channels_first_against_numpy(S):
    """S = 96: less than one column tile; 1024: one full tile of 256 float4; 1028: a tile and one more chunk; 1030, 97: no
    multiple of 4, the one-element path (1030: several tiles)"""
    for C in (1, 3, 7):
        for R in ROWS:
            x = _data(R, C, S, seed=R * 131 + C)
            center = np.round(x.astype(np.float64).mean(axis=(0, 2)), 1)
            for tag, xs in (('clean', x), ('nan', _with_nans(x))):
                mem = _dev(xs)
                for rows in _row_lists(R):
                    for ctr in (None, center):
                        for skipna in ((False,) if tag == 'clean' else (False, True)):
                            got = _abi_moments(mem, R, C, S, sr.strides_channels_first(R, C, S), rows, ctr, skipna)
                            _check_moments(got, xs, rows, ctr, skipna, (S, C, R, tag, rows, ctr is not None, skipna))


def test_moments_where_the_grid_target_sets_the_slab():
    """C = 7, S = 1028: two column tiles per channel, so the 512-workgroup target asks for 37 slabs: 296 rows are 37 slabs of 8
    rows, 297 rows 19 slabs of 16"""
    C, S = 7, 1028
    for R in (295, 296, 297):
        x = _with_nans(_data(R, C, S, seed=R))
        mem = _dev(x)
        for rows in (None, np.arange(R - 1, -1, -1)):
            for skipna in (False, True):
                got = _abi_moments(mem, R, C, S, sr.strides_channels_first(R, C, S), rows, None, skipna)
                _check_moments(got, x, rows, None, skipna, (R, rows is None, skipna))


@pytest.mark.parametrize('C', [4, 7])
def test_moments_channels_last(C):
    R, S = 9, 97
    x = _with_nans(_data(R, C, S, seed=C))
    mem = _dev(x.transpose(0, 2, 1))                                                # (R, S, C) in memory
    center = np.arange(C, dtype=np.float64)
    for skipna in (False, True):
        for rows in _row_lists(R):
            got = _abi_moments(mem, R, C, S, sr.strides_channels_last(R, C, S), rows, center, skipna)
            _check_moments(got, x, rows, center, skipna, ('rows', C, rows, skipna))
        # the row extent folded into S: one row of R * S elements
        folded = x.transpose(1, 0, 2).reshape(1, C, R * S)
        got = _abi_moments(mem, 1, C, R * S, sr.strides_channels_last_folded(R, C, S), None, center, skipna)
        _check_moments(got, folded, None, center, skipna, ('folded', C, skipna))


def test_moments_views_offsets_and_repeatability():
    from DLWP import ops
    R, S = 17, 1028
    x = _data(R, 7, S, seed=1)
    t = _dev(x)
    # a sliced, non-contiguous channels-first view
    got = ops.channel_moments(t[:, 1:6:2], axis=1, as_numpy=True)
    _check_moments(got, x[:, 1:6:2], None, None, False, 'slice')
    # a (T, V, 6, N, N) array and its channels-last twin through the wrapper
    y = _data(9, 3, 6 * 4 * 4, seed=2)
    rows = np.array([8, 0, 3, 3])
    got = ops.channel_moments(_dev(y.reshape(9, 3, 6, 4, 4)), axis=1, rows=rows, center=[1., 2., 3.], as_numpy=True)
    _check_moments(got, y, rows, [1., 2., 3.], False, 'wrapper cf')
    cl = _dev(y.reshape(9, 3, 6, 4, 4).transpose(0, 2, 3, 4, 1))
    got = ops.channel_moments(cl, axis=-1, rows=rows, skipna=True, as_numpy=True)
    _check_moments(got, y, rows, None, True, 'wrapper cl')
    with pytest.raises(IndexError):
        ops.channel_moments(cl, axis=-1, rows=[9])
    # a base pointer 4 bytes past a 16-byte boundary: the one-element path, and still right
    buf = torch.zeros(R * 7 * S + 4, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    off = buf[1:1 + R * 7 * S].view(R, 7, S)
    off.copy_(t)
    assert off.data_ptr() % 16 == 4
    got = ops.channel_moments(off, axis=1, as_numpy=True)
    _check_moments(got, x, None, None, False, 'offset')
    # the same call twice: identical bits, on both load widths
    for src in (t, off):
        a = ops.channel_moments(src, axis=1, center=[0.5] * 7, as_numpy=True)
        b = ops.channel_moments(src, axis=1, center=[0.5] * 7, as_numpy=True)
        assert np.array_equal(a.view(np.int64), b.view(np.int64))
    # nothing selected: zeros, no launch
    assert np.array_equal(ops.channel_moments(t, axis=1, rows=np.zeros(0, np.int64), as_numpy=True), np.zeros((7, 3)))


def test_python_layer_on_the_device_matches_the_host():
    """mean = s1 / n and both sides' s1 lie within n 2^-53 sum|x| of the exact sum: the means differ by at most 2 * 2^-53 sum|x|.
    s2 is a sum of non-negative terms, so its reordering bound is n 2^-53 relative on either side, the root halves it, and the
    shift of the center moves s2 in second order only: stds within 2 n 2^-53 relative (taken twice for the center)."""
    from DLWP.model.preprocessing import mean_by_batch, std_by_batch, variable_statistics
    T, V = 21, 3
    x = _data(T, V, 6 * 8 * 8, seed=9).reshape(T, V, 6, 8, 8)
    t = _dev(x)
    n = x.size // V
    rows = np.arange(2, 19, 2)
    for kw in ({}, {'rows': rows}, {'rows': rows, 'center': [-5., 5., 15.]}):
        mh, sh = variable_statistics(x, **kw)
        md, sd = variable_statistics(t, **kw)
        sel = x if 'rows' not in kw else x[rows]
        bm = 2 * 2.0 ** -53 * np.abs(sel.astype(np.float64)).sum(axis=(0, 2, 3, 4))
        assert np.all(np.abs(md - mh) <= bm), (kw, md - mh, bm)
        assert np.all(np.abs(sd - sh) <= 4 * n * 2.0 ** -53 * sh), (kw, sd - sh)
    xn = x.copy()
    xn[3, 1, 2, 2, 2] = np.nan
    md, sd = variable_statistics(_dev(xn))
    assert np.isnan(md[1]) and np.isnan(sd[1]) and np.isfinite(md[[0, 2]]).all()
    mh, sh = variable_statistics(xn, skipna=True)
    md, sd = variable_statistics(_dev(xn), skipna=True)
    assert np.all(np.abs(md - mh) <= 2 * 2.0 ** -53 * np.nansum(np.abs(xn.astype(np.float64)), axis=(0, 2, 3, 4)))
    assert np.all(np.abs(sd - sh) <= 4 * n * 2.0 ** -53 * sh)
    bm = 2 * 2.0 ** -53 * np.abs(x.astype(np.float64)).sum()
    mh, md = mean_by_batch(x, 4), mean_by_batch(t, 4)
    assert isinstance(md, float) and abs(md - mh) <= bm
    for kw in ({}, {'mean': mh}):
        sh_, sd_ = std_by_batch(x, 4, **kw), std_by_batch(t, 4, **kw)
        assert isinstance(sd_, float) and abs(sd_ - sh_) <= 4 * x.size * 2.0 ** -53 * sh_
    # a permuted view and axis 1 batches give the same numbers
    assert abs(mean_by_batch(t.permute(1, 0, 2, 3, 4), 2, axis=1) - mh) <= bm


# ---- affine -------------------------------------------------------------------------------------------------------------- #

def _tables(C, seed=0):
    rng = np.random.default_rng(100 + seed)
    a = (rng.uniform(0.5, 3., C) * np.where(np.arange(C) % 3 == 1, -1., 1.)).astype(np.float32)      # a negative scale too
    b = rng.uniform(-300., 300., C).astype(np.float32)
    return a, b


def _specials(x):
    """NaN, +-inf, denormals, zeros and the largest finite value in the first elements of the flat array"""
    v = np.array([np.nan, np.inf, -np.inf, 1e-45, -3e-39, 1e-38, 0., -0., 3.4e38, -3.4e38, 1.17549435e-38], dtype=np.float32)
    flat = x.reshape(-1)
    k = min(v.size, flat.size)
    flat[:k] = v[:k]
    flat[-1] = np.float32(5e-41)
    return x


def _abi_affine(src_mem, dst_mem, R, C, S, src, dst, a, b, mode):
    from DLWP import _native as nat
    d = _desc(R, C, S, src, dst)
    return nat.lib().dlwpcs_channel_affine(ctypes.byref(d), src_mem.data_ptr(), a.data_ptr(), b.data_ptr(), mode,
                                           dst_mem.data_ptr(), nat.stream_ptr())


@pytest.mark.parametrize('mode', [sr.MUL_ADD, sr.SUB_DIV])
def test_affine_rows_path_is_numpy_float32_bitwise(mode):
    """channels-first both sides; S = 96: part of a tile, 1028: 257 float4, 4100: a second tile of 1024 float4"""
    from DLWP import ops
    for S in (96, 1028, 4100):
        for R, C in ((3, 3), (1, 7), (2, 64)):
            x = _specials(_data(R, C, S, seed=S + C))
            a, b = _tables(C, seed=C)
            want = sr.affine(x, a, b, mode)
            t = _dev(x)
            got = ops.channel_affine(t, _dev(a), _dev(b), mode, axis=1)
            assert sr.same_bits(got.cpu().numpy(), want), (S, R, C)
            assert sr.same_bits(t.cpu().numpy(), x)                                 # the source is untouched
            assert ops.channel_affine(t, _dev(a), _dev(b), mode, axis=1, out=t) is t
            assert sr.same_bits(t.cpu().numpy(), want), ('in place', S, R, C)


@pytest.mark.parametrize('mode', [sr.MUL_ADD, sr.SUB_DIV])
def test_affine_flat_channels_last_path_is_bitwise(mode):
    """one channels-last stream, channel = index mod C; lengths that are and are not multiples of 4, more than one workgroup
    (4096 elements), C = 3 / 7 (the channel pattern does not repeat with the float4) and C = 64"""
    from DLWP import ops
    for M, C in ((24, 4), (1024, 4), (1371, 3), (601, 7), (2341, 7), (5, 3), (129, 64), (4099, 1)):
        x = _specials(_data(1, C, M, seed=M).transpose(0, 2, 1).copy())            # (1, M, C) in memory
        a, b = _tables(C, seed=M)
        want = sr.affine(x, a, b, mode, axis=2)
        t = _dev(x)
        got = ops.channel_affine(t, _dev(a), _dev(b), mode, axis=-1)
        assert sr.same_bits(got.cpu().numpy(), want), (M, C)
        ops.channel_affine(t, _dev(a), _dev(b), mode, axis=-1, out=t)
        assert sr.same_bits(t.cpu().numpy(), want), ('in place', M, C)
        # the same stream through the C ABI as (R, S) rows back to back, and with the rows folded into S
        R = 3 if M % 3 == 0 else 1
        for Rr, Ss, strides in ((R, M // R, sr.strides_channels_last(R, C, M // R)), (1, M, sr.strides_channels_last_folded(1, C, M))):
            src, dst = _dev(x), torch.zeros(M * C, dtype=torch.float32, device=DEV)
            assert _abi_affine(src, dst, Rr, C, Ss, strides, strides, _dev(a), _dev(b), mode) == 0
            assert sr.same_bits(dst.cpu().numpy().reshape(x.shape), want), (M, C, Rr)


@pytest.mark.parametrize('mode', [sr.MUL_ADD, sr.SUB_DIV])
def test_affine_any_path_changes_the_layout_and_reads_slices(mode):
    from DLWP import ops
    R, C, S = 5, 7, 301
    x = _specials(_data(R, C, S, seed=3))
    a, b = _tables(C, seed=3)
    want = sr.affine(x, a, b, mode)
    da, db = _dev(a), _dev(b)
    cl = _dev(x.transpose(0, 2, 1))                                                 # (R, S, C) in memory
    # channels-last in, channels-first out: lanes along s, a workgroup loops over the channels
    out = torch.zeros(R, C, S, dtype=torch.float32, device=DEV)
    ops.channel_affine(cl, da, db, mode, axis=-1, out=out.permute(0, 2, 1))
    assert sr.same_bits(out.cpu().numpy(), want)
    # channels-first in, channels-last out: lanes along (s, c)
    out = torch.zeros(R, S, C, dtype=torch.float32, device=DEV)
    ops.channel_affine(_dev(x), da, db, mode, axis=1, out=out.permute(0, 2, 1))
    assert sr.same_bits(out.cpu().numpy(), want.transpose(0, 2, 1))
    # sliced sources: every other channel, every other inner element, a row range -- and in place on a view
    t = _dev(x)
    got = ops.channel_affine(t[:, 1:6:2], da[1:6:2], db[1:6:2], mode, axis=1)
    assert got.is_contiguous() and sr.same_bits(got.cpu().numpy(), want[:, 1:6:2])
    got = ops.channel_affine(t[1:4, :, ::2], da, db, mode, axis=1)
    assert sr.same_bits(got.cpu().numpy(), want[1:4, :, ::2])
    view = t[:, :, 1::2]
    ops.channel_affine(view, da, db, mode, axis=1, out=view)
    after = t.cpu().numpy()
    assert sr.same_bits(after[:, :, 1::2], want[:, :, 1::2]) and sr.same_bits(after[:, :, ::2], x[:, :, ::2])
    # a layout the three strides cannot describe goes through contiguous copies
    y = _data(4, 3, 5 * 6, seed=8).reshape(4, 3, 5, 6)
    v = _dev(y)[:, :, ::2, ::2]
    a3, b3 = _tables(3)
    got = ops.channel_affine(v, _dev(a3), _dev(b3), mode, axis=1)
    assert sr.same_bits(got.cpu().numpy(), sr.affine(np.ascontiguousarray(y[:, :, ::2, ::2]), a3, b3, mode))
    # a base pointer off 16 bytes: the one-element path
    buf = torch.zeros(R * C * 300 + 4, dtype=torch.float32, device=DEV)
    off = buf[1:1 + R * C * 300].view(R, C, 300)
    off.copy_(t[:, :, :300])
    x300 = off.cpu().numpy()
    assert off.data_ptr() % 16 == 4
    got = ops.channel_affine(off, da, db, mode, axis=1)
    assert sr.same_bits(got.cpu().numpy(), sr.affine(x300, a, b, mode))


def test_affine_unsupported_descriptor_and_the_fallback():
    from DLWP import _native as nat, ops
    from DLWP.model.preprocessing import VariableScaler
    C = nat.AFFINE_MAX_CHANNELS + 1
    x = _data(2, C, 8, seed=5)
    rng = np.random.default_rng(5)
    mean, std = rng.uniform(-5, 5, C).astype(np.float32), rng.uniform(0.5, 2, C).astype(np.float32)
    t = _dev(x)
    rc = _abi_affine(t, torch.empty_like(t), 2, C, 8, sr.strides_channels_first(2, C, 8), sr.strides_channels_first(2, C, 8),
                     _dev(std), _dev(mean), sr.MUL_ADD)
    assert rc == -2 and b'channel_affine' in nat.lib().dlwpcs_last_error()
    with pytest.raises(NotImplementedError):
        ops.channel_affine(t, _dev(std), _dev(mean), sr.MUL_ADD, axis=1)
    sc = VariableScaler(mean, std)
    assert sr.same_bits(sc.inverse_transform(t).cpu().numpy(), sr.affine(x, std, mean, sr.MUL_ADD))
    assert sr.same_bits(sc.transform(t).cpu().numpy(), sr.affine(x, std, mean, sr.SUB_DIV))
    # bad arguments are refused before any launch
    d = _desc(2, 4, 8, (32, 8, -1), (32, 8, 1))
    assert nat.lib().dlwpcs_channel_affine(ctypes.byref(d), t.data_ptr(), t.data_ptr(), t.data_ptr(), 0, t.data_ptr(), None) == -1
    with pytest.raises(ValueError):
        ops.channel_affine(t, _dev(std[:3]), _dev(mean[:3]), sr.MUL_ADD, axis=1)


# ---- the public layer ---------------------------------------------------------------------------------------------------- #

def test_in_place_preparation_of_a_resident_array():
    """fit, then transform(out=x): the raw array becomes the training array without a second copy.  With z = (x - m) / s the
    scaled statistics are exact up to the float32 tables and the two float32 operations per element: the mean moves by at most
    u |m| / s (the rounded mean table) + 2 u mean|z| (subtraction and division), the std by at most u (the rounded std table)
    + 2 u; the raw data below has |m| / s <= 2, so both stay within 8 u = 8 * 2^-24."""
    from DLWP.model.preprocessing import VariableScaler, variable_statistics
    rng = np.random.default_rng(12)
    raw = rng.standard_normal((12, 2, 6, 8, 8)) * np.array([2., 0.5]).reshape(1, 2, 1, 1, 1) + np.array([3., -1.]).reshape(1, 2, 1, 1, 1)
    raw = raw.astype(np.float32)
    x = _dev(raw)
    ptr = x.data_ptr()
    sc = VariableScaler.fit(x)
    assert sc.transform(x, out=x) is x and x.data_ptr() == ptr
    assert sr.same_bits(x.cpu().numpy(), sr.affine(raw, sc.std, sc.mean, sr.SUB_DIV))
    mean, std = variable_statistics(x)
    print('scaled mean %s std - 1 %s (bound %.3e)' % (mean, std - 1., 8 * U))
    assert np.all(np.abs(mean) <= 8 * U) and np.all(np.abs(std - 1.) <= 8 * U)


def test_end_to_end_unscaled_forecast_at_n8():
    from DLWP.keras import backend
    backend.set_device(DEV)
    from DLWP.model import DLWPFunctional, TimeSeriesEstimator, VariableScaler
    from DLWP.model.cs_unet import build_cs_model
    from DLWP.model.generators import ArrayDataGenerator
    from DLWP.verify import forecast_error
    N, V, T, ITS = 8, 4, 40, 2
    rng = np.random.default_rng(41)
    arr = rng.standard_normal((T, V, 6, N, N)).astype(np.float32)
    sol = rng.random((T, 6, N, N)).astype(np.float32)
    samples = np.arange(0, 12, 3)
    dlwp = DLWPFunctional(is_convolutional=True, time_dim=ITS)
    gen = ArrayDataGenerator(dlwp, arr, rank=3, batch_size=4, input_time_steps=ITS, output_time_steps=ITS, insolation_array=sol,
                             channels_last=True, device=True)
    np.random.seed(0)
    dlwp.build_model(build_cs_model(gen.convolution_shape, ITS * V, 'unet2', base_filter_number=4), loss='mse', optimizer='adam')
    times = np.datetime64('2003-12-25T00') + np.arange(T) * np.timedelta64(6, 'h')
    est = TimeSeriesEstimator(dlwp, gen, sample_times=times)
    # |mean| / std <= 4: the unscaled values carry roundings of u (|mean| + |x| std), small beside differences of order std
    sc = VariableScaler([2., -1.5, 0.5, 3.], [1.5, 0.75, 2.5, 1.25])
    fc = est.predict(4, samples, keep_on_device=True)
    ver = est.verification(4, samples, keep_on_device=True)
    assert fc.values.is_cuda and fc.dims[-1] == 'varlev'
    un = sc.inverse_transform(fc, channels_first=True)
    assert un.values.is_cuda and un.values.is_contiguous() and un.dims == ('f_hour', 'time', 'varlev', 'x0', 'x1', 'x2')
    host = fc.values.cpu().numpy()
    want = (host * sc.std + sc.mean).transpose(0, 1, 5, 2, 3, 4)
    assert sr.same_bits(un.values.cpu().numpy(), want)
    assert sr.same_bits(sc.inverse_transform(fc).values.cpu().numpy(), host * sc.std + sc.mean)
    # rmse of the unscaled pair = std x the scaled rmse, the variable axis kept: both sides are fp32 data reduced in the score
    # kernel's precision -- the tolerance tests/test_gpu_verify_scores.py holds that kernel to
    un_ver = sc.inverse_transform(ver, channels_first=True)
    scaled = forecast_error(fc, ver, 'rmse', axis=(1, 2, 3, 4))
    unscaled = forecast_error(un, un_ver, 'rmse', axis=(1, 3, 4, 5))
    assert scaled.shape == (4, V) and unscaled.shape == (4, V) and np.isfinite(unscaled).all() and (scaled > 0).all()
    print('rmse unscaled %s\n  std x scaled %s' % (unscaled[0], (scaled * sc.std.astype(np.float64))[0]))
    np.testing.assert_allclose(unscaled, scaled * sc.std.astype(np.float64), rtol=1e-5, atol=0.)
