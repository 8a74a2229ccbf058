"""
DLWP.verify's ensemble functions on the host path (numpy in float64) against ensemble_ref.py, their labels, the `axis` and
forecast-hour-first rules, the latitude weights, known values, and every refusal -- those of the device path included, which the
plan query answers on the host.  No device work.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ensemble_ref as R     # noqa: E402

from DLWP import verify as V                         # noqa: E402
from DLWP.model.extensions import Forecast          # noqa: E402

DIMS = ('f_hour', 'time', 'lat', 'lon', 'varlev')
SHAPE = (3, 4, 5, 6, 2)
M = 5


def _labelled(x, dims):
    return Forecast(x, dims, {d: np.arange(n) * 1.5 for d, n in zip(dims, x.shape)})


def _ensemble(rng, holes=True):
    x = (280 + 3 * rng.standard_normal((M,) + SHAPE)).astype(np.float32)
    y = (280 + 3 * rng.standard_normal(SHAPE)).astype(np.float32)
    if holes:
        x[2, 0, 1, 2, 3, 0] = np.nan
        x[4, 1, 0, 0, 0, 1] = np.inf
        y[2, 3, 4, 5, 1] = np.nan
    return x, y


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b)
    assert (np.abs(a - b)[ok] <= tol * np.maximum(1.0, np.abs(b[ok]))).all()


def test_fields_agree_with_the_reference_for_every_member_axis():
    rng = np.random.default_rng(0)
    x, y = _ensemble(rng)
    for ax in range(len(SHAPE) + 1):
        xa = np.moveaxis(x, 0, ax)
        for fair in (False, True):
            ref = R.reference(x, y, fair=fair)
            _close(V.ensemble_crps(xa, y, fair=fair, member_axis=ax), ref['crps'])
        ref = R.reference(x, y)
        _close(V.ensemble_mean(xa, member_axis=ax), ref['mean'])
        _close(V.ensemble_spread(xa, member_axis=ax), ref['spread'])
        _close(V.ensemble_spread(xa, ddof=0, member_axis=ax), R.reference(x, ddof=0)['spread'])
        f = V._ensemble_fields(xa, y, ax, ('rank', 'spread'), variance=True)
        assert f['rank'].dtype == np.int32 and np.array_equal(f['rank'], ref['rank'])
        _close(f['spread'], R.reference(x, variance=True)['spread'])


def test_labels_and_member_dim_by_name():
    rng = np.random.default_rng(1)
    x, y = _ensemble(rng)
    # the member dim in the middle of a labelled input is found by its name
    ens = _labelled(np.moveaxis(x, 0, 2), DIMS[:2] + ('member',) + DIMS[2:])
    val = _labelled(y, DIMS)
    for fn, name in ((lambda: V.ensemble_mean(ens), 'mean'), (lambda: V.ensemble_spread(ens), 'spread'),
                     (lambda: V.ensemble_crps(ens, val), 'crps')):
        out = fn()
        assert isinstance(out, Forecast) and out.dims == DIMS and out.shape == SHAPE
        assert all(np.array_equal(out.coords[d], ens.coords[d]) for d in DIMS) and 'member' not in out.coords
        _close(out.values, R.reference(x, y)[name])
    plain = V.ensemble_crps(np.moveaxis(x, 0, 2), y, member_axis=2)
    assert isinstance(plain, np.ndarray)
    with pytest.raises(ValueError, match='member'):
        V.ensemble_mean(_labelled(x, ('run',) + DIMS))


def test_stack_forecasts():
    rng = np.random.default_rng(2)
    recs = [_labelled(rng.standard_normal(SHAPE).astype(np.float32), DIMS) for _ in range(3)]
    ens = V.stack_forecasts(recs)
    assert ens.dims == ('member',) + DIMS and ens.shape == (3,) + SHAPE and np.array_equal(ens.coords['member'], np.arange(3))
    assert np.array_equal(ens.values[1], recs[1].values) and all(np.array_equal(ens.coords[d], recs[0].coords[d]) for d in DIMS)
    assert V.stack_forecasts(recs, dim='model').dims[0] == 'model'
    other = _labelled(recs[0].values, DIMS)
    other.coords['time'] = other.coords['time'] + 1
    with pytest.raises(ValueError, match='time'):
        V.stack_forecasts([recs[0], other])
    with pytest.raises(ValueError):
        V.stack_forecasts([recs[0], _labelled(recs[0].values, DIMS[:3] + ('x', 'varlev'))])
    with pytest.raises(ValueError):
        V.stack_forecasts([recs[0], recs[0].values])
    with pytest.raises(ValueError):
        V.stack_forecasts([])
    assert V.stack_forecasts([r.values for r in recs]).shape == (3,) + SHAPE


def _host_scores(x, y, w, ax):
    """every method from the reference's fields, in float64"""
    nm = lambda a: V._nanmean(a, ax)      # noqa: E731
    r, rf, rv = R.reference(x, y), R.reference(x, y, fair=True), R.reference(x, variance=True)
    y64 = y.astype(np.float64)
    mse = nm((y64 - r['mean']) ** 2 * w)
    spread = np.sqrt(nm(rv['spread'] * w))
    m = x.shape[0]
    return {'crps': nm(r['crps'] * w), 'fair_crps': nm(rf['crps'] * w), 'spread': spread, 'ens_mse': mse, 'ens_rmse': np.sqrt(mse),
            'ssr': np.sqrt((m + 1.0) / m) * spread / np.sqrt(mse)}


@pytest.mark.parametrize('axis', [None, (1, 2, 3), 2, (0, 4), (1, 2, 3, 4), ()])
def test_ensemble_error_axis_lead_first_and_weights(axis):
    rng = np.random.default_rng(3)
    x, y = _ensemble(rng)
    ens, val = _labelled(x, ('member',) + DIMS), _labelled(y, DIMS)
    lat = np.linspace(-80, 80, SHAPE[2])
    val.lat = Forecast(lat, ('lat',), {'lat': val.coords['lat']})
    w = np.cos(np.deg2rad(lat))
    w = (w / w.mean()).reshape(1, 1, -1, 1, 1)
    ax = tuple(range(1, len(SHAPE))) if axis is None else ((axis,) if isinstance(axis, int) else tuple(axis))
    for weighted in (False, True):
        want = _host_scores(x, y, w if weighted else 1.0, ax)
        for method in V._ENS_METHODS:
            got = V.ensemble_error(ens, val, method, axis=axis, weighted=weighted)
            assert got.dtype == np.float64
            if 0 not in ax:
                assert got.shape[0] == SHAPE[0]
            _close(got, want[method], 1e-11)
    # the mean-error methods ARE forecast_error of the ensemble mean
    for method in ('mse', 'rmse'):
        direct = V.forecast_error(V.ensemble_mean(ens), val, method, axis=axis, weighted=True)
        assert np.array_equal(direct, V.ensemble_error(ens, val, 'ens_' + method, axis=axis, weighted=True), equal_nan=True)


def test_valid_broadcasts_over_unit_dims():
    rng = np.random.default_rng(4)
    x, y = _ensemble(rng, holes=False)
    y1 = y[:, :1]
    got = V.ensemble_crps(x, y1)
    _close(got, R.reference(x, np.broadcast_to(y1, SHAPE).copy())['crps'])


def test_rank_histogram():
    rng = np.random.default_rng(5)
    x, y = _ensemble(rng)
    rank = R.reference(x, y)['rank']
    h = V.rank_histogram(x, y)
    assert h.dtype == np.int64 and h.shape == (M + 1,)
    assert np.array_equal(h, np.bincount(rank[rank >= 0], minlength=M + 1)) and h.sum() == (rank >= 0).sum() == rank.size - 3
    h = V.rank_histogram(_labelled(x, ('member',) + DIMS), _labelled(y, DIMS), axis=(1, 2, 3))
    assert h.dims == ('f_hour', 'varlev', 'rank') and h.shape == (SHAPE[0], SHAPE[4], M + 1)
    for f in range(SHAPE[0]):
        for v in range(SHAPE[4]):
            r = rank[f, :, :, :, v]
            assert np.array_equal(h.values[f, v], np.bincount(r[r >= 0], minlength=M + 1))


def test_known_values():
    # M identical members: spread 0, crps = |x - y|
    x0 = np.array([280.25, -3.0, 0.0], np.float32)
    y = np.array([281.0, -3.0, 5.5], np.float32)
    x = np.broadcast_to(x0, (7, 3)).copy()
    assert np.array_equal(V.ensemble_spread(x), np.zeros(3)) and np.array_equal(V.ensemble_mean(x), x0.astype(np.float64))
    for fair in (False, True):
        assert np.array_equal(V.ensemble_crps(x, y, fair=fair), np.abs(x0.astype(np.float64) - y))
    # two members {a, b} with y between them: (b - a) / 4 in the standard form, 0 in the fair form
    a, b = 1.0, 3.5
    two = np.array([[a], [b]], np.float32).reshape(2, 1, 1)
    yy = np.array([[2.0]], np.float32)
    assert V.ensemble_error(two, yy, 'crps', axis=())[0, 0] == (b - a) / 4
    assert V.ensemble_error(two, yy, 'fair_crps', axis=())[0, 0] == 0.0
    # y far outside: crps -> |mean - y| - B / 2
    three = np.array([1.0, 2.0, 4.0], np.float32).reshape(3, 1)
    got = V.ensemble_crps(three, np.array([10.0], np.float32))[0]
    assert abs(got - ((9 + 8 + 6) / 3 - (2 * (1 + 3 + 2)) / 9 / 2)) < 1e-14


def test_spread_skill_ratio_of_an_exchangeable_ensemble():
    """members and verification drawn from one distribution per element (a random centre plus unit noise): E (x-bar - y)^2 =
    (M + 1) / M sigma^2, so ssr -> 1.  n = 200000 elements, M = 10: ssr^2 is a ratio of two means whose relative standard
    errors are sqrt(2 / (n (M - 1))) and sqrt(2 / n); together below 0.0034, half of it for the root: a standard error of
    0.0017 -- the tolerance 0.01 is more than five of them."""
    n, m = 200000, 10
    rng = np.random.default_rng(11)
    centre = 280 + 5 * rng.standard_normal(n)
    x = (centre + rng.standard_normal((m, n))).astype(np.float32).reshape(m, 1, n)
    y = (centre + rng.standard_normal(n)).astype(np.float32).reshape(1, n)
    ssr = V.ensemble_error(x, y, 'ssr')
    assert ssr.shape == (1,) and abs(ssr[0] - 1.0) < 0.01
    # an under-dispersive ensemble (members share half of the verification's variance) is well below 1
    x2 = (centre + 0.5 * rng.standard_normal((m, n))).astype(np.float32).reshape(m, 1, n)
    assert V.ensemble_error(x2, y, 'ssr')[0] < 0.6
    # and its rank histogram is U-shaped where the exchangeable one is flat
    flat, ushape = V.rank_histogram(x, y), V.rank_histogram(x2, y)
    assert flat.sum() == ushape.sum() == n
    assert np.abs(flat / (n / (m + 1.0)) - 1).max() < 0.05 and ushape[0] > 2 * ushape[m // 2]


def test_refusals():
    rng = np.random.default_rng(6)
    x, y = _ensemble(rng, holes=False)
    with pytest.raises(ValueError, match='at least 2'):
        V.ensemble_mean(x[:1])
    with pytest.raises(ValueError, match='at least 2'):
        V.ensemble_error(x[:1], y, 'crps')
    with pytest.raises(NotImplementedError, match='lagged'):
        V.ensemble_crps(x, y[0])                                       # a continuous series: one axis fewer
    with pytest.raises(NotImplementedError, match='lagged'):
        V.rank_histogram(x, y[0])
    with pytest.raises(ValueError):
        V.ensemble_crps(x, y[:, :2])                                   # neither 1 nor the extent
    with pytest.raises(ValueError, match='method'):
        V.ensemble_error(x, y, 'rmse')
    ens, val = _labelled(x, ('member',) + DIMS), _labelled(y, DIMS)
    with pytest.raises(ValueError, match='dims'):
        V.ensemble_crps(ens, _labelled(y, DIMS[:3] + ('x', 'varlev')))
    val.coords['lat'] = val.coords['lat'] + 0.5
    with pytest.raises(ValueError, match='lat'):
        V.ensemble_error(ens, val, 'crps')
    with pytest.raises(ValueError):
        V.ensemble_mean(x, member_axis=9)


def test_device_path_refusals_answered_on_the_host():
    from DLWP import ops
    assert ops.ENSEMBLE_MAX_M == R.MAX_M == 128
    assert ops.ensemble_plan((128, 8), (8, 1))['m_class'] == 128
    with pytest.raises(NotImplementedError, match='128'):
        ops.ensemble_plan((129, 8), (8, 1))
    with pytest.raises(ValueError, match='at least 2'):
        ops.ensemble_plan((1, 8), (8, 1))
    with pytest.raises(ValueError):
        ops.ensemble_plan((4, 8), (8, 1), valid_shape=(3,), valid_strides=(1,))
    with pytest.raises(ValueError, match='ddof'):
        ops.ensemble_plan((4, 8), (8, 1), ddof=2)
    with pytest.raises(ValueError, match='aligned'):
        ops.ensemble_plan((4, 8), (8, 1), ens_ptr=(1 << 20) + 2)
    import torch
    from DLWP import _native as nat
    with pytest.raises(nat.NativeError):
        ops.ensemble_stats(torch.zeros(4, 8), want=('mean',))         # no CPU fallback behind the device entry
    # unit dims are dropped and adjacent dims merged: one merged dim for a contiguous ensemble
    assert ops.ensemble_layout((3, 1, 5, 1, 8), (40, 40, 8, 8, 1), 0)[4] == [(40, (1, 0))]
    assert ops.ensemble_layout((3, 5, 8), (40, 8, 1), 0, (5, 8), (8, 1))[4] == [(40, (1, 1))]
