"""
GPU tests of dlwpcs_time_spectrum (csrc/time_spectrum.hip) through DLWP.ops and DLWP.verify: the three forms against the float64
reference of tests/time_spectrum_ref.py within its derived bound, every element compared and the counts exactly; the bit claims
(pair quantity 0 = single form, every split, with and without counts, twice); missing values; short series; layouts; a tile list
longer than 65536; one case out of exact-size, poisoned, guarded memory; the verify functions on device tensors.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hostile_mem as H          # noqa: E402
import time_spectrum_ref as R    # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _inside(got, want, lim, what):
    """every element: both NaN, or |got - want| <= lim"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    lim = np.broadcast_to(lim, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), '%s: NaN pattern' % what
    err = np.where(nan, 0.0, np.abs(got - want))
    worst = np.where(nan, 0.0, err - lim)
    assert np.all(worst <= 0.0), '%s: |error| %.3e against the bound %.3e at %s' % (
        what, err.flat[np.argmax(worst)], lim.flat[np.argmax(worst)], np.unravel_index(np.argmax(worst), want.shape))


def _check_all_forms(x, y, M, hop, w, detrend, n_freq, min_count=1, split=None):
    """single, pair and coefficient form of (T, C) host arrays against the reference; returns the device results"""
    from DLWP import ops
    K = R.clip_freq(n_freq, M)
    xd, yd = _dev(x), _dev(y)
    one = R.reference(x, M, hop, w, detrend, K, min_count)
    two = R.reference(x, M, hop, w, detrend, K, min_count, b=y)
    p, cnt = ops.time_spectrum(xd, None, M, hop, w, detrend=detrend, n_freq=K, min_count=min_count, split=split, counts=True)
    assert p.shape == (K, x.shape[1]) and np.array_equal(cnt.cpu().numpy(), one['count'])
    _inside(p.cpu().numpy(), one['power'][0], R.bound(M, one['m'], 1)[0], 'power')
    q, cnt2 = ops.time_spectrum(xd, yd, M, hop, w, detrend=detrend, n_freq=K, min_count=min_count, split=split, counts=True)
    assert q.shape == (4, K, x.shape[1]) and np.array_equal(cnt2.cpu().numpy(), two['count'])
    _inside(q.cpu().numpy(), two['power'], R.bound(M, two['m'], 4), 'pair')
    z = ops.time_fourier(xd, M, hop, w, detrend=detrend, n_freq=K).cpu().numpy()
    assert z.shape == (one['coef'].shape[0], K, 2, x.shape[1])
    lim = R.bound_coef(M, np.nan_to_num(one['sum_abs']))
    _inside(z[:, :, 0], one['coef'].real, lim, 'Re X')
    _inside(z[:, :, 1], one['coef'].imag, lim, 'Im X')
    return p, q, cnt, cnt2


@pytest.mark.parametrize('M', R.GPU_M)
def test_forms_against_the_reference(M):
    i = R.GPU_M.index(M)
    for j, hop in enumerate(R.hops(M)):
        ncol = R.COLUMNS[(i + j) % len(R.COLUMNS)]
        n_freq = R.N_FREQ[(i + 2 * j) % len(R.N_FREQ)]
        kind = R.WINDOWS[(i + j) % len(R.WINDOWS)]
        detrend = bool((i + j // 2) % 2)
        rng = np.random.default_rng(1000 * M + hop)
        T = R.rows_for(M, hop)
        x, y = R.make_series(rng, T, ncol, offset=1.0), R.make_series(rng, T, ncol, offset=-0.5)
        p, q, _, _ = _check_all_forms(x, y, M, hop, R.window(kind, M, rng), detrend, n_freq)
        assert np.array_equal(_bits(q[0]), _bits(p)), 'pair quantity 0 is not the single form (M %d, hop %d)' % (M, hop)


def test_the_case_table_covers_every_value():
    seen = set()
    for i, M in enumerate(R.GPU_M):
        for j in range(4):
            seen |= {('c', R.COLUMNS[(i + j) % 6]), ('f', R.N_FREQ[(i + 2 * j) % 5]), ('w', R.WINDOWS[(i + j) % 3]), ('d', (i + j // 2) % 2)}
    assert len(seen) == 6 + 5 + 3 + 2


@pytest.mark.parametrize('n_seg', (1, R.SLAB - 1, R.SLAB, R.SLAB + 1, 2 * R.SLAB + 1))
@pytest.mark.parametrize('ncol', (33, 260))
def test_bit_claims(n_seg, ncol):
    from DLWP import ops
    M, hop = 32, 16
    rng = np.random.default_rng(n_seg * ncol)
    T = R.rows_for(M, hop, n_seg)
    x, y = R.make_series(rng, T, ncol, 1.0), R.make_series(rng, T, ncol)
    x[T // 2, 3] = np.nan
    w = R.window('hann', M)
    p, q, cnt, cnt2 = _check_all_forms(x, y, M, hop, w, True, None)
    xd, yd = _dev(x), _dev(y)
    assert ops.time_spectrum_plan(xd.shape, xd.stride(), M, hop)['slabs'] == -(-n_seg // R.SLAB)
    for split in (False, True, None):
        p2 = ops.time_spectrum(xd, None, M, hop, w, detrend=True, split=split)
        q2, c2 = ops.time_spectrum(xd, yd, M, hop, w, detrend=True, split=split, counts=True)
        assert np.array_equal(_bits(p2), _bits(p)), 'single form, split %r' % (split,)
        assert np.array_equal(_bits(q2), _bits(q)) and np.array_equal(c2.cpu().numpy(), cnt2.cpu().numpy()), 'pair form, split %r' % (split,)
    assert np.array_equal(_bits(q[0]), _bits(p))
    a, b = ops.time_fourier(xd, M, hop, w, detrend=True), ops.time_fourier(xd, M, hop, w, detrend=True)
    assert np.array_equal(_bits(a), _bits(b))


def test_missing_values_and_min_count():
    from DLWP import ops
    M, hop, T, ncol = 8, 6, 27, 40                       # segments 0-7, 6-13, 12-19, 18-25; row 26 is left over
    rng = np.random.default_rng(77)
    x, y = R.make_series(rng, T, ncol), R.make_series(rng, T, ncol)
    xb, yb = x.view(np.uint32), y.view(np.uint32)
    for i, bits in enumerate(R.NAN_BITS):
        xb[0, i] = bits                                  # the first row of segment 0
        xb[25, 6 + i] = bits                             # the last row of segment 3
        xb[6, 12 + i] = bits                             # a row that segments 0 and 1 share
        yb[13, 18 + i] = bits                            # the second operand only: the last row of segment 1, shared with segment 2
    for r in (0, 8, 14, 20):
        xb[r, 30] = R.NAN_BITS[r % 6]                    # no segment counts
    xb[26, 31] = R.NAN_BITS[0]                           # the row left over: every segment counts
    w = R.window('random', M, rng)
    for detrend in (False, True):
        for mc in (1, 2, 3, 4):
            p, q, cnt, cnt2 = _check_all_forms(x, y, M, hop, w, detrend, None, min_count=mc)
            c, c2 = cnt.cpu().numpy(), cnt2.cpu().numpy()
            assert c[:6].tolist() == [3] * 6 and c[6:12].tolist() == [3] * 6 and c[12:18].tolist() == [2] * 6 and c[18:24].tolist() == [4] * 6
            assert c2[18:24].tolist() == [2] * 6 and c[30] == 0 and c2[30] == 0 and c[31] == 4
            pn = np.isnan(p.cpu().numpy())
            assert pn[:, 30].all() and pn[:, 12].all() == (mc > 2) and pn[:, 0].all() == (mc > 3) and not pn[:, 31].any()
            assert np.all(_bits(p)[pn] == 0x7FC00000)
    xd = _dev(x)
    a, c = ops.time_spectrum(xd, None, M, hop, w, counts=True)
    b = ops.time_spectrum(xd, None, M, hop, w)
    assert np.array_equal(_bits(a), _bits(b))            # with and without counts


def test_short_series():
    from DLWP import ops
    rng = np.random.default_rng(3)
    M = 16
    x = R.make_series(rng, M, 37)
    xd = _dev(x)
    w = R.window('hann', M)
    for pair in (False, True):
        p, cnt = ops.time_spectrum(xd[:M - 1], xd[:M - 1] if pair else None, M, 8, w, counts=True)
        assert p.shape == ((4, 9, 37) if pair else (9, 37)) and np.all(_bits(p) == 0x7FC00000) and not cnt.any()
    assert ops.time_fourier(xd[:M - 1], M, 8, w).shape == (0, 9, 2, 37)
    p, q, cnt, _ = _check_all_forms(x, x[::-1].copy(), M, 8, w, True, None)      # T == M: one segment
    assert np.all(cnt.cpu().numpy() == 1)


def test_layouts():
    from DLWP import ops
    M, hop, T = 16, 8, 43
    rng = np.random.default_rng(9)
    x = R.make_series(rng, T, 6 * 20, 0.5)
    x[5, 7] = np.nan
    y = R.make_series(rng, T, 6 * 20)
    w = R.window('hann', M)
    base, baseq, cnt, _ = _check_all_forms(x, y, M, hop, w, True, None)
    base, baseq, cnt = _bits(base).reshape(9, 6, 20), _bits(baseq).reshape(4, 9, 6, 20), cnt.cpu().numpy().reshape(6, 20)
    zb = _bits(ops.time_fourier(_dev(x), M, hop, w, detrend=True)).reshape(4, 9, 2, 6, 20)
    x3, y3 = _dev(x.reshape(T, 6, 20)), _dev(y.reshape(T, 6, 20))

    def run(a, b, axis, out_perm=None):
        p, c = ops.time_spectrum(a, None, M, hop, w, row_axis=axis, detrend=True, out_perm=out_perm, counts=True)
        q = ops.time_spectrum(a, b, M, hop, w, row_axis=axis, detrend=True, out_perm=out_perm)
        z = ops.time_fourier(a, M, hop, w, row_axis=axis, detrend=True, out_perm=out_perm)
        return _bits(p), _bits(q), c.cpu().numpy(), _bits(z)

    # the row axis not first, in a contiguous array
    p, q, c, z = run(x3.permute(1, 0, 2).contiguous(), y3.permute(1, 0, 2).contiguous(), 1)
    assert np.array_equal(p, base.transpose(1, 0, 2)) and np.array_equal(q, baseq.transpose(0, 2, 1, 3)) and np.array_equal(c, cnt)
    assert np.array_equal(z, zb.transpose(0, 3, 1, 2, 4))
    # a permuted view: the lanes run along a strided dim
    p, q, c, z = run(x3.permute(2, 0, 1), y3.permute(2, 0, 1), 1)
    assert np.array_equal(p, base.transpose(2, 0, 1)) and np.array_equal(q, baseq.transpose(0, 3, 1, 2)) and np.array_equal(c, cnt.T)
    assert np.array_equal(z, zb.transpose(0, 4, 1, 2, 3))
    # out_perm: the frequencies last
    p, q, c, z = run(x3, y3, 0, out_perm=(1, 2, 0))
    assert np.array_equal(p, base.transpose(1, 2, 0)) and np.array_equal(q, baseq.transpose(0, 2, 3, 1)) and np.array_equal(c, cnt)
    assert np.array_equal(z, zb.transpose(0, 3, 4, 1, 2))
    # a view offset by one element: no 16-byte loads
    fx, fy = torch.empty(x3.numel() + 1, device=DEV), torch.empty(x3.numel() + 1, device=DEV)
    fx[1:].copy_(x3.reshape(-1)), fy[1:].copy_(y3.reshape(-1))
    assert ops.time_spectrum_plan(x3.shape, x3.stride(), M, hop)['vec']
    p, q, c, z = run(fx[1:].view(T, 6, 20), fy[1:].view(T, 6, 20), 0)
    assert np.array_equal(p, base) and np.array_equal(q, baseq) and np.array_equal(c, cnt) and np.array_equal(z, zb)
    # inner stride 2: interleaved complex
    xy = torch.stack([x3, y3], dim=-1)
    p, q, c, z = run(xy[..., 0], xy[..., 1], 0)
    assert np.array_equal(p, base) and np.array_equal(q, baseq) and np.array_equal(c, cnt) and np.array_equal(z, zb)
    # a unit-stride row axis (the zonal use)
    xt, yt = x3.permute(1, 2, 0).contiguous(), y3.permute(1, 2, 0).contiguous()
    p, q, c, z = run(xt, yt, 2)
    assert np.array_equal(p, base.transpose(1, 2, 0)) and np.array_equal(q, baseq.transpose(0, 2, 3, 1)) and np.array_equal(c, cnt)
    assert np.array_equal(z, zb.transpose(0, 3, 4, 1, 2))
    # a stride-0 axis
    p, q, c, z = run(x3[:, :1].expand(T, 3, 20), y3[:, :1].expand(T, 3, 20), 0)
    assert np.array_equal(p, base[:, [0, 0, 0]]) and np.array_equal(q, baseq[:, :, [0, 0, 0]]) and np.array_equal(c, cnt[[0, 0, 0]])
    assert np.array_equal(z, zb[:, :, :, [0, 0, 0]])


def test_tile_list_beyond_65536():
    """T = M = 2 over 65537 * 32 + 5 columns: 65538 column tiles, the last one partial.  Every column against the closed form
    X_0 = x_0 + x_1, X_1 = x_0 - x_1, P_f = |X_f|^2 / 4, m = (x_0^2 + x_1^2) / 2 within bound(); the columns at the seam of
    65536 tiles and the last ones bitwise against the same columns computed alone."""
    from DLWP import ops
    ncol = 65537 * 32 + 5
    plan = ops.time_spectrum_plan((2, ncol), (ncol, 1), 2)
    assert plan['tiles'] == 65538 > 65536 and plan['col_tiles'] == 65538 and plan['grid'] < plan['tiles'] and not plan['vec']
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    xd = torch.randn(2, ncol, device=DEV, generator=g)
    p, cnt = ops.time_spectrum(xd, None, 2, counts=True)
    assert p.shape == (2, ncol) and bool((cnt == 1).all())
    x = xd.cpu().numpy().astype(np.float64)
    want = np.stack([(x[0] + x[1]) ** 2, (x[0] - x[1]) ** 2]) / 4.0
    lim = 4.0 * (2 + R.C) * R.EPS * (x ** 2).sum(axis=0) / 2.0
    _inside(p.cpu().numpy(), want, lim[None, :], 'power over 65538 tiles')
    for lo, hi in ((65536 * 32 - 40, 65536 * 32 + 40), (ncol - 40, ncol)):
        alone = ops.time_spectrum(xd[:, lo:hi].contiguous(), None, 2)
        assert np.array_equal(_bits(alone), _bits(p[:, lo:hi]))
    z = ops.time_fourier(xd, 2)
    assert z.shape == (1, 2, 2, ncol)
    _inside(z[0, :, 0].cpu().numpy(), np.stack([x[0] + x[1], x[0] - x[1]]), ((2 + R.C_COEF) * R.EPS * np.abs(x).sum(axis=0))[None, :], 'Re X')


def test_out_of_exact_size_poisoned_guarded_memory():
    from DLWP import ops
    from DLWP import _native as nat
    arena = H.Arena(64 << 20, DEV)
    rng = np.random.default_rng(21)
    M, hop, ncol, K = 33, 5, 70, 9
    T = R.rows_for(M, hop, 2 * R.SLAB + 3)
    x, y = R.make_series(rng, T, ncol, 1.0), R.make_series(rng, T, ncol)
    x[40, 3] = np.inf
    w32 = R.window('hann', M)
    sw = float((w32.astype(np.float64) ** 2).sum())
    a, b = arena.place(_dev(x), 'a'), arena.place(_dev(y), 'b')
    win, tw = arena.place(_dev(w32), 'window'), arena.place(_dev(R.twiddle(M)), 'twiddle')
    lib, stream = nat.lib(), torch.cuda.current_stream().cuda_stream
    one, two = R.reference(x, M, hop, w32, True, K), R.reference(x, M, hop, w32, True, K, b=y)
    n_seg = R.n_segments(T, M, hop)
    for pair in (False, True):
        for split in (0, 1):
            d, oshape = ops.rows_layout(a.shape, a.stride(), 0, None, K)
            out = arena.tensor(([4] if pair else []) + list(oshape), torch.float32, name='power')
            cnt = arena.tensor((ncol,), torch.int32, name='counts')
            nbytes = int(lib.dlwpcs_time_spectrum_scratch_bytes(ctypes.byref(d), T, M, hop, K, int(pair), split))
            assert (nbytes > 0) == bool(split)
            scratch = arena.carve(nbytes, name='scratch') if nbytes else None
            with torch.cuda.device(a.device):
                nat.check(lib.dlwpcs_time_spectrum(ctypes.byref(d), a.data_ptr(), b.data_ptr() if pair else None, T, M, hop, win.data_ptr(),
                                                   tw.data_ptr(), sw, 1, K, 1, 0, split, K * ncol, 0, out.data_ptr(), cnt.data_ptr(),
                                                   scratch.data_ptr() if nbytes else None, nbytes, stream), 'dlwpcs_time_spectrum')
            arena.assert_guards()
            assert not bool(H.is_poison(cnt).any()), 'a count was never written'
            ref = two if pair else one
            assert np.array_equal(cnt.cpu().numpy(), ref['count'])
            _inside(out.cpu().numpy().reshape(ref['power'].shape), ref['power'], R.bound(M, ref['m'], 4 if pair else 1), 'guarded power')
    d, oshape = ops.rows_layout(a.shape, a.stride(), 0, None, 2 * K)
    part = int(d.out_row_stride)
    d.out_row_stride = 2 * part
    z = arena.tensor([n_seg] + list(oshape), torch.float32, name='coefficients')
    with torch.cuda.device(a.device):
        nat.check(lib.dlwpcs_time_spectrum(ctypes.byref(d), a.data_ptr(), None, T, M, hop, win.data_ptr(), tw.data_ptr(), sw, 1, K, 1, 1, -1,
                                           2 * K * ncol, part, z.data_ptr(), None, None, 0, stream), 'dlwpcs_time_spectrum')
    arena.assert_guards()
    zh = z.cpu().numpy().reshape(n_seg, K, 2, ncol)
    lim = R.bound_coef(M, np.nan_to_num(one['sum_abs']))
    _inside(zh[:, :, 0], one['coef'].real, lim, 'guarded Re X')
    _inside(zh[:, :, 1], one['coef'].imag, lim, 'guarded Im X')


def test_argument_errors_on_the_device():
    from DLWP import ops
    x = torch.zeros(40, 8, device=DEV)
    with pytest.raises(NotImplementedError):
        ops.time_spectrum(torch.zeros(2000, 4, device=DEV), None, 1729)
    for kw in (dict(n_segment=1), dict(n_segment=16, hop=0), dict(n_segment=16, n_freq=10), dict(n_segment=16, min_count=0),
               dict(n_segment=16, window=np.ones(15)), dict(n_segment=16, window=np.zeros(16))):
        with pytest.raises(ValueError):
            ops.time_spectrum(x, None, **kw)
    with pytest.raises(TypeError):
        ops.time_spectrum(x, x[:, :4], 16)
    with pytest.raises(TypeError):
        ops.time_spectrum(x.double(), None, 16)


# ---- the verify functions on device tensors ----------------------------------------------------------------------------- #

def test_verify_functions_against_their_host_path():
    from DLWP import verify as V
    from DLWP.model.extensions import Forecast
    M, hop, T = 24, 12, 75
    rng = np.random.default_rng(31)
    x = R.make_series(rng, T, 5 * 7).reshape(T, 5, 7)
    y = R.make_series(rng, T, 5 * 7).reshape(T, 5, 7)
    x[30, 2, 3] = np.nan
    w = R.window('hann', M)
    ref = R.reference(x.reshape(T, -1), M, hop, w, True, b=y.reshape(T, -1))
    one = R.reference(x.reshape(T, -1), M, hop, w, True)
    # the host path subtracts the unrounded mean: |mean| 2^-24 per value, which moves P by at most 4 sqrt(m) |mean| 2^-24
    mean_a = np.abs(np.nan_to_num(x)).reshape(T, -1).max(axis=0)                 # (at least any segment's |mean|)
    extra = 4.0 * np.sqrt(one['m'][0]) * mean_a * R.EPS + 2.0 * (mean_a * R.EPS) ** 2
    xd, yd = _dev(x), _dev(y)
    hp, hc = V.time_spectrum(x, M, return_count=True)
    dp, dc = V.time_spectrum(xd, M, return_count=True)
    assert dp.is_cuda and dp.dtype == torch.float32 and np.array_equal(dc.cpu().numpy(), hc)
    _inside(dp.cpu().numpy().reshape(13, -1), hp.reshape(13, -1), R.bound(M, one['m'], 1)[0] + extra[None, :], 'time_spectrum')
    mean_b = np.abs(y).reshape(T, -1).max(axis=0)
    extra4 = 4.0 * R.EPS * (np.sqrt(ref['m'][0]) + np.sqrt(ref['m'][1])) * (mean_a + mean_b)
    hcs = V.time_cross_spectrum(x, y, M)
    dcs = V.time_cross_spectrum(xd, yd, M)
    lim = R.bound(M, ref['m'], 4) + extra4[None, None, :]
    for i in range(4):
        _inside(dcs[i].cpu().numpy().reshape(13, -1), hcs[i].reshape(13, -1), lim[i], 'time_cross_spectrum %d' % i)
    hcoh, dcoh = V.time_coherence(x, y, M, n_freq=6), V.time_coherence(xd, yd, M, n_freq=6)
    # d coh <= (2 |cross| d cross / (Pa Pb)) + coh (dPa / Pa + dPb / Pb), every d from the bounds above
    with np.errstate(invalid='ignore', divide='ignore'):
        pa, pb = hcs.power_a.reshape(13, -1)[:6], hcs.power_b.reshape(13, -1)[:6]
        cross = np.sqrt(hcs.co.reshape(13, -1)[:6] ** 2 + hcs.quad.reshape(13, -1)[:6] ** 2)
        tol = 2.0 * cross * 1.5 * lim[2] / (pa * pb) + hcoh.reshape(6, -1) * (lim[0] / pa + lim[1] / pb) + 8 * R.EPS
    _inside(dcoh.cpu().numpy().reshape(6, -1), hcoh.reshape(6, -1), 1.1 * np.nan_to_num(tol), 'time_coherence')
    hz, dz = V.time_fourier(x, n_segment=M, hop=hop, window='hann'), V.time_fourier(xd, n_segment=M, hop=hop, window='hann')
    assert dz.is_cuda and dz.dtype == torch.complex64 and tuple(dz.shape) == hz.shape == (5, 13, 5, 7)
    flat = R.reference(x.reshape(T, -1), M, hop, w, False)
    climit = R.bound_coef(M, np.nan_to_num(flat['sum_abs']))
    dzh = dz.cpu().numpy().reshape(5, 13, -1)
    _inside(dzh.real, hz.reshape(5, 13, -1).real, climit, 'time_fourier Re')
    _inside(dzh.imag, hz.reshape(5, 13, -1).imag, climit, 'time_fourier Im')
    whole = V.time_fourier(xd[:40])
    assert tuple(whole.shape) == (21, 5, 7)
    fc = Forecast(xd.permute(1, 0, 2), ('lat', 'time', 'lon'), {'time': np.arange(T), 'lat': np.arange(5.), 'lon': np.arange(7.)})
    lab = V.time_spectrum(fc, M)
    assert lab.dims == ('lat', 'frequency', 'lon') and lab.values.is_cuda
    assert np.array_equal(_bits(lab.values), _bits(dp.permute(1, 0, 2)))


def test_wavenumber_frequency_spectrum_on_the_device():
    """
    Device against host path.  With S = sum_f (eastward + westward) of the host path = (m_a + m_b) c_k / L^2 (Parseval), the time
    stage moves (P_aa + P_bb) / 2 +- Q by at most 4 (M + C) 2^-24 (m_a + m_b), that is 4 (M + C) 2^-24 S after the scaling.  The
    zonal stage hands it a, b with |da|, |db| <= d1 = (L + C_COEF) 2^-24 max_t sum_lon |x|, which moves a power by at most
    4 sqrt(m) d1 + d1^2 per operand (|X_f| <= sqrt(M S_w m), |dX_f| <= sqrt(M S_w) d1, c_f <= 2) and the mean the host subtracts
    unrounded by 2^-24 |mean| more per value; the elementwise fp32 combination adds 8 * 2^-24 S.
    """
    from DLWP import verify as V
    M, hop, L, T = 32, 16, 20, 80
    k0, f0 = 3, 5
    t = np.arange(T)[:, None, None]
    lon = 2.0 * np.pi * np.arange(L)[None, None, :] / L
    amp = np.array([0.5, 1.0, 2.0])[None, :, None]
    rng = np.random.default_rng(41)
    wave = (amp * np.cos(k0 * lon - 2.0 * np.pi * f0 * t / M)).astype(np.float32)
    noise = R.make_series(rng, T, 3 * L).reshape(T, 3, L)
    noise[50, 1, 4] = np.nan
    for x, kw in ((wave, dict(window='boxcar', detrend=None, hop=M)), (wave, dict()), (noise, dict()),
                  (noise, dict(component='antisymmetric', lat_axis=1, n_wave=4, n_freq=7))):
        (he, hw), hc = V.wavenumber_frequency_spectrum(x, M, return_count=True, **kw)
        (de, dw), dc = V.wavenumber_frequency_spectrum(_dev(x), M, return_count=True, **kw)
        assert de.is_cuda and tuple(de.shape) == he.shape and np.array_equal(dc.cpu().numpy(), hc)
        full = V.wavenumber_frequency_spectrum(x, M, **dict(kw, n_freq=None))
        S = np.nansum(full.eastward + full.westward, axis=0, keepdims=True)[..., :he.shape[-1]]
        ck = np.where(np.arange(he.shape[-1]) == 0, 1.0, 2.0) * np.where(2 * np.arange(he.shape[-1]) == L, 0.5, 1.0) / L ** 2
        absx = np.abs(np.nan_to_num(x)).sum(axis=-1).max(axis=0)[None, :, None]
        d1 = ((L + R.C_COEF) + 2.0) * R.EPS * absx          # (+ the mean, + the fp32 mirror combination)
        m_ab = S / ck
        lim = 4.0 * (M + R.C) * R.EPS * S + ck * (2.0 * (4.0 * np.sqrt(m_ab) * d1 + d1 ** 2)) + 8.0 * R.EPS * S
        _inside(de.cpu().numpy(), he, lim, 'eastward')
        _inside(dw.cpu().numpy(), hw, lim, 'westward')
        if x is wave:
            e, w_ = de.cpu().numpy().astype(np.float64), dw.cpu().numpy().astype(np.float64)
            assert np.all(np.abs(w_[f0, :, k0]) <= lim[0, :, k0])                          # nothing travels westward
            assert np.all(e[f0, :, k0] > 0.6 * S[0, :, k0])                                # (Hann keeps 2 / 3 in the central bin)
            if 'window' in kw:                                                             # Parseval on the device
                total = (e + w_).sum(axis=(0, 2))
                want = (wave.astype(np.float64) ** 2).mean(axis=(0, 2))
                assert np.all(np.abs(total - want) <= lim.sum(axis=(0, 2)) * e.shape[0] * 2)
