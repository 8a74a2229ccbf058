"""
The time-axis filters of DLWP.verify on the host: lanczos_weights, time_filter, running_mean and lead_window_mean on numpy and
labelled inputs -- shapes, dims, coordinates under every label, mode, missing-value rule and min_count, and the errors.  No device.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import time_filter_ref as R     # noqa: E402

from DLWP import verify                             # noqa: E402
from DLWP.model.extensions import Forecast          # noqa: E402


def _series(T=60, shape=(3, 4), seed=0, holes=0.1):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(T,) + shape) * 5. + 270.
    x[rng.random(x.shape) < holes] = np.nan
    times = np.datetime64('2001-01-01T00') + np.arange(T) * np.timedelta64(6, 'h')
    return x, times


# --------------------------------------------------------------------------------------------------------------------- #
# lanczos_weights
# --------------------------------------------------------------------------------------------------------------------- #

def _lanczos(n, fc):
    """the formula restated: w_k = 2 fc sinc(2 fc k) sinc(k / (n + 1)), sinc(x) = sin(pi x) / (pi x), normalised to sum 1"""
    k = np.arange(-n, n + 1, dtype=np.float64)

    def sinc(v):
        out = np.ones_like(v)
        nz = v != 0
        out[nz] = np.sin(np.pi * v[nz]) / (np.pi * v[nz])
        return out
    w = 2. * fc * sinc(2. * fc * k) * sinc(k / (n + 1.))
    return w / w.sum()


@pytest.mark.parametrize('n,fc,fh', ((1, 0.25, None), (10, 1. / 24., None), (60, 1. / 24., 1. / 8.), (60, 0.01, 0.5), (7, 0.1, 0.3)))
def test_lanczos_weights(n, fc, fh):
    w = verify.lanczos_weights(n, fc, fh)
    assert w.dtype == np.float64 and w.shape == (2 * n + 1,)
    assert np.array_equal(w, w[::-1])                                                   # symmetric to the last bit
    want = _lanczos(n, fc) if fh is None else _lanczos(n, fh) - _lanczos(n, fc)
    assert abs(w.sum() - (1. if fh is None else 0.)) <= 1e-15
    assert np.all(np.abs(w - want) <= 1e-14)
    assert np.all(w != 0.)
    if fh is None:
        # a low-pass: the response at frequency 0 is 1, and it falls to about a half at the cut-off
        k = np.arange(-n, n + 1)
        assert abs((w * np.cos(2. * np.pi * fc * k)).sum() - 0.5) < 0.1


def test_lanczos_weights_refuses():
    for args in ((0, 0.1), (5, 0.), (5, 0.6), (5, 0.2, 0.1), (5, 0.2, 0.2), (5, 0.2, 0.7)):
        with pytest.raises(ValueError):
            verify.lanczos_weights(*args)


# --------------------------------------------------------------------------------------------------------------------- #
# time_filter / running_mean
# --------------------------------------------------------------------------------------------------------------------- #

@pytest.mark.parametrize('K,step', ((1, 1), (5, 1), (5, 2), (28, 4), (28, 28), (3, 7)))
def test_time_filter_on_numpy_matches_the_definition(K, step):
    x, _ = _series()
    T = x.shape[0]
    w = np.random.default_rng(K).random(K) + 0.1
    flat = x.reshape(T, -1)
    for mode in ('valid', 'same'):
        o, J = ((K - 1) // 2 if mode == 'same' else 0), R.n_out(T, K, step, mode)
        num, ab, den, n = R.filter_exact(flat, w, step, o, J)
        out, cnt = verify.time_filter(x, w, step=step, mode=mode, return_count=True)
        assert out.shape == (J,) + x.shape[1:] and out.dtype == np.float64 and cnt.dtype == np.int32
        assert np.array_equal(cnt.reshape(J, -1), n)
        assert np.array_equal(np.isnan(out.reshape(J, -1)), n < K)
        ok = n == K
        assert np.allclose(out.reshape(J, -1)[ok], num[ok], rtol=1e-13, atol=0.)
        out = verify.time_filter(x, w, step=step, mode=mode, missing='skip', min_weight=0.6)
        with np.errstate(all='ignore'):
            want = np.where(den >= 0.6 * w.sum() * (1 - 1e-15), num / den, np.nan)
        edge = np.abs(den - 0.6 * w.sum()) < 1e-12                                      # (none: the weights are random)
        assert not edge.any()
        assert np.array_equal(np.isnan(out.reshape(J, -1)), np.isnan(want))
        assert np.allclose(out.reshape(J, -1), want, rtol=1e-13, atol=0., equal_nan=True)
    # another axis
    moved = np.moveaxis(x, 0, 1)
    a = verify.time_filter(moved, w, axis=1, step=step)
    assert np.array_equal(np.moveaxis(a, 1, 0), verify.time_filter(x, w, step=step), equal_nan=True)


def test_all_present_passes_at_min_weight_one():
    x, _ = _series(holes=0.)
    for K in (3, 10, 28, 61):
        w = np.random.default_rng(K).random(K) + 0.01
        out = verify.time_filter(x, w, missing='skip', min_weight=1.0)
        assert not np.isnan(out).any()
        x2 = x.copy()
        x2[K // 2, 0, 0] = np.nan
        out = verify.time_filter(x2, w, missing='skip', min_weight=1.0)
        assert np.isnan(out[:, 0, 0]).sum() == min(K // 2 + 1, out.shape[0]) and not np.isnan(out[:, 1:]).any()


def test_running_mean_is_the_rolling_mean():
    x, _ = _series(T=50, holes=0.2)
    for n, step, mc in ((4, 1, None), (4, 1, 1), (4, 2, 3), (28, 4, 20), (7, 7, None)):
        out, cnt = verify.running_mean(x, n, step=step, min_count=mc, return_count=True)
        J = (50 - n) // step + 1
        assert out.shape == (J, 3, 4)
        for j in range(J):
            win = x[j * step:j * step + n]
            k = (~np.isnan(win)).sum(axis=0)
            assert np.array_equal(cnt[j], k)
            with np.errstate(all='ignore'):
                want = np.where(k >= (n if mc is None else mc), np.nansum(win, axis=0) / k, np.nan)
            assert np.allclose(out[j], want, rtol=1e-14, atol=0., equal_nan=True)
    same = verify.running_mean(x, 5, mode='same', min_count=1)
    assert same.shape == x.shape
    with np.errstate(all='ignore'):
        assert np.allclose(same[0], np.nansum(x[:3], axis=0) / (~np.isnan(x[:3])).sum(axis=0), rtol=1e-14, equal_nan=True)
    for bad in (dict(n=0), dict(n=4, min_count=0), dict(n=4, min_count=5), dict(n=4, step=0), dict(n=4, mode='full'),
                dict(n=4, label='middle')):
        with pytest.raises(ValueError):
            verify.running_mean(x, **bad)
    assert verify.running_mean(x, 51).shape == (0, 3, 4)


def test_labelled_inputs_keep_their_labels():
    x, times = _series(T=40)
    ds = Forecast(np.moveaxis(x, 0, 1), ('face', 'time', 'cell'), {'time': times, 'face': np.arange(3), 'cell': np.arange(4)})
    ds.lat = 'the latitudes'
    for label, at in (('end', 27), ('centre', 13), ('start', 0), (None, 27)):
        out = verify.running_mean(ds, 28, step=4, label=label)
        assert isinstance(out, Forecast) and out.dims == ds.dims and out.shape == (3, 4, 4) and out.lat == 'the latitudes'
        assert np.array_equal(out.coords['time'], times[at::4][:4]) and np.array_equal(out.coords['cell'], np.arange(4))
        assert np.array_equal(out.values, verify.running_mean(ds.values, 28, axis=1, step=4), equal_nan=True)
    w = verify.lanczos_weights(3, 0.2)
    out, cnt = verify.time_filter(ds, w, mode='same', step=3, return_count=True)
    assert out.dims == cnt.dims == ds.dims and out.shape == (3, 14, 4) and np.array_equal(out.coords['time'], times[::3])
    assert np.array_equal(cnt.coords['time'], times[::3]) and cnt.values.dtype == np.int32
    assert cnt.values[0, 0, 0] <= 4 and cnt.values.max() == 7
    for label in ('end', 'start'):
        with pytest.raises(ValueError):
            verify.time_filter(ds, w, mode='same', label=label)
    # by name, by position; a labelled input without a 'time' dim filters axis 0
    assert np.array_equal(verify.time_filter(ds, w, axis='time').values, verify.time_filter(ds, w, axis=1).values, equal_nan=True)
    other = Forecast(x, ('sample', 'face', 'cell'), {'sample': np.arange(40)})
    out = verify.time_filter(other, w)
    assert out.shape == (34, 3, 4) and np.array_equal(out.coords['sample'], np.arange(6, 40)) and 'face' not in out.coords
    for bad in (dict(axis='lead'), dict(axis=3), dict(missing='drop'), dict(mode='full')):
        with pytest.raises(ValueError):
            verify.time_filter(ds, w, **bad)
    with pytest.raises(ValueError):
        verify.time_filter(ds, [1., -1.], missing='skip')
    with pytest.raises(ValueError):
        verify.time_filter(ds, [1., np.nan])
    with pytest.raises(ValueError):
        verify.time_filter(ds, [])


def test_lead_window_mean_against_numpy():
    rng = np.random.default_rng(4)
    f = rng.normal(size=(24, 5, 6)).astype(np.float32)
    f[rng.random(f.shape) < 0.2] = np.nan
    lead = np.arange(24) * 6
    win = ((8, 12), (12, 16), (16, 24))
    fc = Forecast(f, ('f_hour', 'time', 'cell'), {'f_hour': lead, 'time': np.arange(5), 'cell': np.arange(6)})
    for mc in (None, 1, (4, 2, 5)):
        out = verify.lead_window_mean(fc, win, min_count=mc)
        assert out.dims == fc.dims and out.shape == (3, 5, 6) and out.values.dtype == np.float32
        assert np.array_equal(out.coords['f_hour'], [66, 90, 138]) and np.array_equal(out.coords['time'], np.arange(5))
        for i, (a, b) in enumerate(win):
            k = (~np.isnan(f[a:b])).sum(axis=0)
            need = (b - a) if mc is None else np.broadcast_to(mc, (3,))[i]
            with np.errstate(all='ignore'):
                want = np.where(k >= need, np.nansum(f[a:b].astype(np.float64), axis=0) / k, np.nan).astype(np.float32)
            assert np.array_equal(out.values[i], want, equal_nan=True)
    plain = verify.lead_window_mean(np.moveaxis(f, 0, 2), win, axis=2, min_count=1)
    assert plain.shape == (5, 6, 3) and np.array_equal(np.moveaxis(plain, 2, 0), verify.lead_window_mean(fc, win, min_count=1).values,
                                                       equal_nan=True)
    for bad in (((0, 0),), ((5, 3),), ((0, 25),), ((-1, 3),), ()):
        with pytest.raises(ValueError):
            verify.lead_window_mean(fc, bad)
    with pytest.raises(ValueError):
        verify.lead_window_mean(fc, win, min_count=5)
