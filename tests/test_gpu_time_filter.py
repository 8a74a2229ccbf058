"""
dlwpcs_time_filter on the device against the float32 restatement of time_filter_ref.py, bit for bit, counts included, no element
left out: both forms do the header's additions in tap order, so nothing is left to a tolerance.  (K, s) pairs in every
accumulator class, on both sides of each class boundary and beyond the last; series that are no multiple of the step, shorter
than the taps and exactly as long; forced slab lengths; every origin; element sets around a lane, a chunk and a column tile;
layouts that cannot merge, permuted views, out_perm and a view offset by one element; hostile data.  One case runs out of
exact-size poisoned guarded memory.  The verify functions on device inputs against their host path.
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
import time_filter_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T0, E0 = 97, 1028                # 97 rows: a multiple of no step but 1; 1028 elements: 257 chunks, 5 scalar column tiles


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope='module')
def series():
    x = R.make_series(np.random.default_rng(11), T0, E0)
    return x, torch.from_numpy(x).to(DEV)


def _geometry(T, K, s, mode):
    return ((K - 1) // 2 if mode == 'same' else 0), R.n_out(T, K, s, mode)


def _check(xd, x, h, s, o, J, mode, mw=0., form=None, slab=None, what=''):
    """one launch with counts against the reference: (value bits, counts) of the device"""
    from DLWP import ops
    got, cnt = ops.time_filter(xd, h, step=s, origin=o, n_out=J, mode='mean' if mode else 'sum', min_weight=mw, form=form,
                               slab_rows=slab, counts=True)
    want, n = R.filter_ref(x.reshape(x.shape[0], -1), np.asarray(h, dtype=np.float32), s, o, J, mode, mw)
    got, cnt = got.cpu().numpy().reshape(J, -1), cnt.cpu().numpy().reshape(J, -1)
    diff = _bits(got) != _bits(want)
    assert not diff.any(), '%s: %d of %d values differ, first at %s' % (what, int(diff.sum()), diff.size, np.argwhere(diff)[0])
    assert cnt.dtype == np.int32 and np.array_equal(cnt, n), '%s: counts' % what
    return _bits(got), cnt


@pytest.mark.parametrize('i', range(len(R.KS_CASES)))
def test_every_class_in_both_modes_forms_and_at_slab_seams(series, i):
    from DLWP import ops
    K, s = R.KS_CASES[i]
    x, xd = series
    rng = np.random.default_rng(100 + i)
    streams = R.n_live(K, s) <= R.MAX_CLASS
    for mode, geo in ((R.SUM, ('valid', 'same')[i % 2]), (R.MEAN, ('same', 'valid')[i % 2])):
        h = R.make_taps(rng, K, positive=mode == R.MEAN)
        o, J = _geometry(T0, K, s, geo)
        what = 'K %d s %d mode %d %s' % (K, s, mode, geo)
        ref = _check(xd, x, h, s, o, J, mode, 0.3 * float(h.sum()), what=what)
        for form, slab in ((None, 3), ('gather', None), ('gather', 5)) + ((('streaming', 1), ('streaming', None)) if streams else ()):
            got = _check(xd, x, h, s, o, J, mode, 0.3 * float(h.sum()), form, slab, what + ' form %s slab %s' % (form, slab))
            assert np.array_equal(got[0], ref[0])
        # without counts: another instantiation, the same bits
        plain = ops.time_filter(xd, h, step=s, origin=o, n_out=J, mode='mean' if mode else 'sum', min_weight=0.3 * float(h.sum()))
        assert np.array_equal(_bits(plain.cpu().numpy().reshape(J, -1)), ref[0]), what + ' without counts'
    if streams:
        assert ops.time_filter_plan((T0, E0), (E0, 1), K, step=s, form='streaming')['a_class'] == R.plan(K, s, 10, E0, True, R.STREAMING)[1]
    else:
        with pytest.raises(ValueError):
            ops.time_filter(xd, h, step=s, form='streaming')


@pytest.mark.parametrize('T', (3, 5, 40, 130))
def test_series_shorter_than_as_long_as_and_longer_than_the_taps(T):
    from DLWP import ops
    rng = np.random.default_rng(T)
    x = R.make_series(rng, T, 260)
    xd = torch.from_numpy(x).to(DEV)
    for K, s in ((5, 2), (9, 1), (40, 3)):
        h = R.make_taps(rng, K, positive=True)
        for geo in ('valid', 'same'):
            o, J = _geometry(T, K, s, geo)
            if J == 0:
                assert T < K and geo == 'valid'
                out, cnt = ops.time_filter(xd, h, step=s, counts=True)
                assert tuple(out.shape) == (0, 260) and tuple(cnt.shape) == (0, 260)
                continue
            for mode in (R.SUM, R.MEAN):
                _check(xd, x, h, s, o, J, mode, what='T %d K %d s %d %s mode %d' % (T, K, s, geo, mode))


@pytest.mark.parametrize('K,s', ((9, 2), (28, 1), (28, 4), (61, 1)))
def test_forced_slab_lengths_and_forms_give_the_same_bits(series, K, s):
    x, xd = series
    h = R.make_taps(np.random.default_rng(K), K, positive=True)
    o, J = _geometry(T0, K, s, 'same')
    forms = ('streaming', 'gather', None) if R.n_live(K, s) <= R.MAX_CLASS else ('gather', None)
    for mode in (R.SUM, R.MEAN):
        seen = [_check(xd, x, h, s, o, J, mode, 1.5, form, slab, 'K %d s %d form %s slab %s' % (K, s, form, slab))[0]
                for form in forms for slab in (1, 3, 7, 10, J, J + 5)]
        assert (J % 7 or J % 10) and all(np.array_equal(b, seen[0]) for b in seen)


def test_min_weight_at_below_and_above_an_attainable_weight(series):
    x, xd = series
    f = np.float32
    h = np.ones(5, f)
    o, J = _geometry(T0, 5, 1, 'same')
    kept = []
    for mw in (f(3.), np.nextafter(f(3.), f(0.)), np.nextafter(f(3.), f(4.)), f(0.), f(5.), np.nextafter(f(5.), f(6.))):
        got, cnt = _check(xd, x, h, 1, o, J, R.MEAN, float(mw), what='min_weight %r' % mw)
        kept.append(int((got != R.QNAN).sum()))
        assert np.all((got != R.QNAN) <= (cnt >= float(mw)))
    assert kept[0] == kept[1] > kept[2] > kept[4] > kept[5] == 0 and kept[3] > kept[0]


def test_every_origin(series):
    x, xd = series
    h = R.make_taps(np.random.default_rng(5), 5)
    for s in (1, 2):
        for o in range(5):
            for mode in (R.SUM, R.MEAN):
                _check(xd, x, np.abs(h) if mode else h, s, o, -(-T0 // s), mode, what='origin %d step %d' % (o, s))


@pytest.mark.parametrize('E', R.E_CASES)
def test_element_sets_around_a_lane_a_chunk_and_a_tile(E):
    rng = np.random.default_rng(E)
    x = R.make_series(rng, 43, E)
    xd = torch.from_numpy(x).to(DEV)
    for K, s in ((5, 2), (28, 1), (3, 4), (40, 1)):
        h = R.make_taps(rng, K, positive=True)
        o, J = _geometry(43, K, s, 'same')
        for mode in (R.SUM, R.MEAN):
            _check(xd, x, h, s, o, J, mode, 1., what='E %d K %d s %d' % (E, K, s))
            _check(xd, x, h, s, o, J, mode, 1., form='streaming' if R.n_live(K, s) <= R.MAX_CLASS else 'gather', slab=4,
                   what='E %d K %d s %d slab 4' % (E, K, s))


def test_layouts_views_and_out_perm():
    from DLWP import ops
    rng = np.random.default_rng(3)
    T, C, Y, X = 41, 3, 6, 12
    x = R.make_series(rng, T, C * Y * X).reshape(T, C, Y, X)
    xd = torch.from_numpy(x).to(DEV)
    h = R.make_taps(rng, 7, positive=True)                  # classes 8 and 4: 16-byte chunks where the layout allows
    for s, mode in ((1, 'sum'), (2, 'mean'), (1, 'mean')):
        J = R.n_out(T, 7, s, 'same')
        want, n = R.filter_ref(x.reshape(T, -1), h, s, 3, J, mode == 'mean', 2.)
        want, n = want.reshape(J, C, Y, X), n.reshape(J, C, Y, X)

        def run(src, **kw):
            out, cnt = ops.time_filter(src, h, step=s, origin=3, n_out=J, mode=mode, min_weight=2., counts=True, **kw)
            return out.cpu().numpy(), cnt.cpu().numpy()
        out, cnt = run(xd)
        assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(cnt, n)
        # two inner dims that cannot merge: the last dim cut from a wider one, 16-byte chunks (8) and single elements (7)
        for cut in (8, 7):
            out, cnt = run(xd[..., :cut])
            assert np.array_equal(_bits(out), _bits(want[..., :cut])) and np.array_equal(cnt, n[..., :cut])
        # the time axis in the middle of a permuted view; channels-first into channels-last
        view = xd.permute(1, 0, 2, 3)
        assert not view.is_contiguous()
        out, cnt = run(view, row_axis=1)
        assert np.array_equal(_bits(out), _bits(want.transpose(1, 0, 2, 3))) and np.array_equal(cnt, n.transpose(1, 0, 2, 3))
        out, cnt = run(xd, out_perm=(0, 2, 3, 1))
        assert out.shape == (J, Y, X, C)
        assert np.array_equal(_bits(out), _bits(want.transpose(0, 2, 3, 1))) and np.array_equal(cnt, n.transpose(0, 2, 3, 1))
        # the same data one element off the 16-byte grid: the scalar path on what otherwise takes 16-byte chunks
        flat = torch.empty(xd.numel() + 1, dtype=torch.float32, device=DEV)
        flat[1:].copy_(xd.reshape(-1))
        off = flat[1:].view(xd.shape)
        assert off.data_ptr() % 16 == 4 and xd.data_ptr() % 16 == 0
        assert ops.time_filter_plan(xd.shape, xd.stride(), 7, step=s)['vec']
        assert not ops.time_filter_plan(xd.shape, xd.stride(), 7, step=s, aligned=False)['vec']
        out, cnt = run(off)
        assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(cnt, n)


@pytest.mark.parametrize('K,s,form', ((28, 1, 'streaming'), (28, 4, None), (5, 7, None), (40, 1, None), (9, 2, 'gather')))
def test_out_of_exact_size_poisoned_guarded_memory(K, s, form):
    from DLWP import ops
    from DLWP import _native as nat
    arena = H.Arena(64 << 20, DEV)
    rng = np.random.default_rng(K + s)
    T, E = 53, 516
    x = R.make_series(rng, T, E)
    h = R.make_taps(rng, K, positive=True)
    src = arena.place(torch.from_numpy(x).to(DEV), 'series')
    taps = arena.place(torch.from_numpy(h).to(DEV), 'taps')
    for mode in (R.SUM, R.MEAN):
        for geo in ('valid', 'same'):
            o, J = _geometry(T, K, s, geo)
            d, oshape = ops.rows_layout(src.shape, src.stride(), 0, None, J)
            out = arena.tensor(oshape, torch.float32, name='filtered')
            cnt = arena.tensor(oshape, torch.int32, name='counts')
            with torch.cuda.device(src.device):
                nat.check(nat.lib().dlwpcs_time_filter(ctypes.byref(d), src.data_ptr(), T, taps.data_ptr(), K, s, o, J, mode,
                                                       ctypes.c_float(1.), {None: -1, 'streaming': 0, 'gather': 1}[form], 3, out.data_ptr(),
                                                       cnt.data_ptr(), torch.cuda.current_stream().cuda_stream),
                          'dlwpcs_time_filter')
            arena.assert_guards()
            assert not bool(H.is_poison(cnt).any()), 'a count was never written'
            want, n = R.filter_ref(x, h, s, o, J, mode, 1.)
            assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)) and np.array_equal(cnt.cpu().numpy(), n)


def test_twice_the_same_bits_and_bad_arguments(series):
    from DLWP import ops
    x, xd = series
    h = R.make_taps(np.random.default_rng(2), 28)
    a = ops.time_filter(xd, h, origin=13, n_out=T0)
    b = ops.time_filter(xd, torch.from_numpy(h).to(DEV), origin=13, n_out=T0)
    assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))
    with pytest.raises(ValueError):
        ops.time_filter(xd, h, mode='mean')                         # taps of both signs
    with pytest.raises(ValueError):
        ops.time_filter(xd, h, origin=28)
    with pytest.raises(ValueError):
        ops.time_filter(xd, np.ones(R.MAX_TAPS + 1))
    with pytest.raises(ValueError):
        ops.time_filter(xd, [1., np.inf])
    with pytest.raises(TypeError):
        ops.time_filter(xd.double(), h)
    with pytest.raises(TypeError):
        ops.time_filter(xd, torch.from_numpy(h))                    # device data, host tensor of taps


def test_verify_functions_on_the_device_against_their_host_path():
    from DLWP import verify
    from DLWP.model.extensions import Forecast
    rng = np.random.default_rng(8)
    T, E = 120, 37
    x = R.make_series(rng, T, E)
    times = np.datetime64('2001-01-01T00') + np.arange(T) * np.timedelta64(6, 'h')
    host = Forecast(x, ('time', 'cell'), {'time': times, 'cell': np.arange(E)})
    dev = Forecast(torch.from_numpy(x).to(DEV), ('time', 'cell'), {'time': times, 'cell': np.arange(E)})

    def same(a, b):
        assert a.dims == b.dims and all(np.array_equal(a.coords[d], b.coords[d]) for d in a.dims) and set(a.coords) == set(b.coords)
        va, vb = a.values.cpu().numpy(), np.asarray(b.values)
        assert va.shape == vb.shape and va.dtype == np.float32 and np.array_equal(np.isnan(va), np.isnan(vb))
        return va, vb

    w = verify.lanczos_weights(10, 1. / 24., 1. / 8.)
    for mode in ('valid', 'same'):
        a, b = verify.time_filter(dev, w, mode=mode), verify.time_filter(host, w, mode=mode)
        va, vb = same(a, b)
        o, J = _geometry(T, len(w), 1, mode)
        _, ab, _, _ = R.filter_exact(x, w.astype(np.float32), 1, o, J)
        ok = ~np.isnan(va) & np.isfinite(vb)
        # the host path uses the float64 weights: their rounding to float32 is one more relative u on every term
        assert ok.any() and np.all(np.abs(va - vb)[ok] <= (R.bound_sum(len(w), ab) + R.gamma(1) * ab)[ok])
    for step, mc in ((1, None), (4, 20), (28, 1)):
        (a, na), (b, nb) = (verify.running_mean(v, 28, step=step, min_count=mc, return_count=True) for v in (dev, host))
        va, vb = same(a, b)
        assert np.array_equal(na.values.cpu().numpy(), nb.values) and na.values.dtype == torch.int32
        J = R.n_out(T, 28, step, 'valid')
        _, ab, den, n = R.filter_exact(x, np.ones(28, np.float32), step, 0, J)
        ok = ~np.isnan(va) & np.isfinite(vb)
        assert ok.any() and np.all(np.abs(va - vb)[ok] <= R.bound_mean(28, ab, den)[ok])
        assert np.all(~np.isnan(va) <= (n >= (mc or 28)))
    a = verify.time_filter(dev, np.ones(5) / 5., mode='same', missing='skip', min_weight=0.6)
    b = verify.time_filter(host, np.ones(5) / 5., mode='same', missing='skip', min_weight=0.6)
    same(a, b)
    # the lead axis of a forecast: unequal windows through the grouped mean
    f = R.make_series(rng, 24, 3 * E).reshape(24, 3, E)
    lead = np.arange(24) * 6
    fh = Forecast(f, ('f_hour', 'time', 'cell'), {'f_hour': lead, 'time': times[:3], 'cell': np.arange(E)})
    fd = Forecast(torch.from_numpy(f).to(DEV), fh.dims, fh.coords)
    win = ((0, 4), (4, 12), (10, 24))
    a, b = verify.lead_window_mean(fd, win, min_count=(4, 6, 10)), verify.lead_window_mean(fh, win, min_count=(4, 6, 10))
    assert a.dims == b.dims and np.array_equal(a.coords['f_hour'], [18, 66, 138]) and np.array_equal(b.coords['f_hour'], [18, 66, 138])
    assert np.array_equal(_bits(a.values.cpu().numpy()), _bits(b.values))
