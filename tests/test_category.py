"""
DLWP.verify's categorical ensemble scores on the host path (numpy in float64) against category_ref.py, their labels, the threshold
dim by name, the `axis` and forecast-hour-first rules, the latitude weights, the identities between the scores, the reliability
counts, and every refusal -- those of the device path included, which the plan query answers on the host.  No device work.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import category_ref as R     # noqa: E402

from DLWP import verify as V                         # noqa: E402
from DLWP.model.extensions import Forecast          # noqa: E402

DIMS = ('f_hour', 'time', 'lat', 'lon', 'varlev')
SHAPE = (3, 4, 5, 6, 2)
M, Q = 5, 2
F = np.float32


def _labelled(x, dims):
    return Forecast(x, dims, {d: np.arange(n) * 1.5 for d, n in zip(dims, x.shape)})


def _ensemble(rng, holes=True, q=Q):
    """values on a grid of 0.25: members and verifications sit on thresholds"""
    g = lambda a: (280 + np.round(4 * a) / 4).astype(F)      # noqa: E731
    x, y = g(rng.standard_normal((M,) + SHAPE)), g(rng.standard_normal(SHAPE))
    t = np.sort(g(0.7 * rng.standard_normal((q,) + SHAPE)), axis=0)
    if holes:
        x[2, 0, 1, 2, 3, 0] = np.nan
        x[4, 1, 0, 0, 0, 1] = np.inf
        y[2, 3, 4, 5, 1] = np.nan
        t[-1, 0, 0, 1, 1, 1] = np.nan
    return x, y, t


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b)
    assert (np.abs(a - b)[ok] <= tol * np.maximum(1.0, np.abs(b[ok]))).all()


def test_fields_agree_with_the_reference_for_every_member_and_threshold_axis():
    rng = np.random.default_rng(0)
    x, y, t = _ensemble(rng)
    rp = R.ref_probs(Q)
    for fair in (False, True):
        ref = R.reference(x, y, t, fair, rp)
        for ax in range(len(SHAPE) + 1):
            xa, ta = np.moveaxis(x, 0, ax), np.moveaxis(t, 0, ax)
            _close(V.ranked_probability_score(xa, y, ta, fair=fair, member_axis=ax, threshold_axis=ax), ref['rps'])
            if fair:
                continue
            _close(V.ensemble_probability(xa, ta, member_axis=ax, threshold_axis=ax), ref['prob'])
            _close(V.brier_score(xa, y, ta, member_axis=ax, threshold_axis=ax), ref['brier'])
            f = V._category_fields(xa, y, ta, ax, ax, ('code', 'rps_ref'), ref_prob=rp)
            assert f['code'].dtype == np.int32 and np.array_equal(f['code'], ref['code'])
            _close(f['rps_ref'], ref['rps_ref'])
    assert (x[:, None] == t[None]).any() and (y[None] == t).any()                 # the inputs do hit the thresholds


def test_a_bare_threshold_vector_and_broadcast_thresholds():
    rng = np.random.default_rng(1)
    x, y, _ = _ensemble(rng)
    vec = np.array([279.75, 280.25, 280.25], dtype=F)
    ref = R.reference(x, y, vec.reshape((3,) + (1,) * len(SHAPE)))
    _close(V.brier_score(x, y, vec), ref['brier'])
    _close(V.brier_score(x, y, [279.75, 280.25, 280.25]), ref['brier'])
    _close(V.ranked_probability_score(np.moveaxis(x, 0, 2), y, vec, member_axis=2), ref['rps'])
    per_lat = (280 + np.arange(5) * 0.25).astype(F).reshape(1, 1, 1, 5, 1, 1)
    _close(V.ensemble_probability(x, per_lat), R.reference(x, None, np.broadcast_to(per_lat, (1,) + SHAPE))['prob'])


def test_labels_and_the_threshold_dim_by_name():
    rng = np.random.default_rng(2)
    x, y, t = _ensemble(rng)
    ens, val = _labelled(np.moveaxis(x, 0, 2), DIMS[:2] + ('member',) + DIMS[2:]), _labelled(y, DIMS)
    for name in ('quantile', 'threshold'):
        thr = Forecast(np.moveaxis(t, 0, 1), DIMS[:1] + (name,) + DIMS[1:], dict(val.coords, **{name: np.array([1 / 3, 2 / 3])}))
        ref = R.reference(x, y, t)
        p = V.ensemble_probability(ens, thr, member_axis=5, threshold_axis=4)          # the names win over the arguments
        assert isinstance(p, Forecast) and p.dims == (name,) + DIMS and np.array_equal(p.coords[name], [1 / 3, 2 / 3])
        assert np.array_equal(p.coords['lat'], val.coords['lat']) and p.name == 'ensemble_probability'
        _close(p.values, ref['prob'])
        b = V.brier_score(ens, val, thr)
        assert b.dims == (name,) + DIMS and b.name == 'brier_score'
        _close(b.values, ref['brier'])
        r = V.ranked_probability_score(ens, val, thr)
        assert r.dims == DIMS and 'member' not in r.coords and name not in r.coords
        _close(r.values, ref['rps'])
    assert not isinstance(V.brier_score(x, y, t), Forecast)
    with pytest.raises(ValueError, match="'quantile'"):
        V.brier_score(ens, val, _labelled(t, ('q',) + DIMS))
    with pytest.raises(ValueError, match='do not match'):
        V.brier_score(ens, val, Forecast(t, ('quantile',) + DIMS[:3] + ('x', 'varlev'), {}))


def test_quantile_table_through_the_time_series_feeds_the_scores():
    """climatology_quantiles -> daily_climo_time_series (also lazy) -> brier_score: the threshold dim sits behind f_hour"""
    rng = np.random.default_rng(3)
    n = 2 * 365
    times = np.datetime64('2001-01-01') + np.arange(n).astype('timedelta64[D]')
    hist = Forecast((280 + 3 * rng.standard_normal((n, 4, 2))).astype(F), ('time', 'x', 'varlev'),
                    {'time': times, 'x': np.arange(4), 'varlev': np.arange(2)})
    table = V.climatology_quantiles(hist, (1 / 3, 2 / 3))
    when = times[[10, 200, 364]]
    f_hour = np.array([0, 24])
    dims = ('f_hour', 'time', 'x', 'varlev')
    co = {'f_hour': f_hour, 'time': when, 'x': np.arange(4), 'varlev': np.arange(2)}
    x = (280 + 3 * rng.standard_normal((M, 2, 3, 4, 2))).astype(F)
    y = (280 + 3 * rng.standard_normal((2, 3, 4, 2))).astype(F)
    ens, val = Forecast(x, ('member',) + dims, dict(co, member=np.arange(M))), Forecast(y, dims, co)
    series = V.daily_climo_time_series(table, when, f_hour)
    t = np.moveaxis(series.values, 1, 0)
    ref = R.reference(x, y, t, ref_prob=np.array([1 / 3, 2 / 3]))
    for thr in (series, V.daily_climo_time_series(table, when, f_hour, lazy=True)):
        b = V.brier_score(ens, val, thr)
        assert b.dims == ('quantile',) + dims and np.allclose(b.coords['quantile'], [1 / 3, 2 / 3])
        _close(b.values, ref['brier'])
        s = V.categorical_error(ens, val, thr, 'rpss', probabilities=(1 / 3, 2 / 3))
        assert s.shape == (2,)
        _close(s, 1 - ref['rps'].mean(axis=(1, 2, 3)) / ref['rps_ref'].mean(axis=(1, 2, 3)))


@pytest.mark.parametrize('axis', [None, (1, 2, 3), (0, 2), 4, (-1, 1)])
def test_categorical_error_axis_lead_first_and_weights(axis):
    rng = np.random.default_rng(4)
    x, y, t = _ensemble(rng)
    ens, val = _labelled(x, ('member',) + DIMS), _labelled(y, DIMS)
    lat = Forecast(np.linspace(-80, 80, 5), ('lat',), {})
    val.lat = lat
    w = np.cos(np.deg2rad(lat.values))
    w = (w / w.mean()).reshape(1, 1, 5, 1, 1)
    ax = tuple(range(1, 5)) if axis is None else tuple(a % 5 for a in (axis if isinstance(axis, tuple) else (axis,)))
    rp = (0.3, 0.7)
    for fair in (False, True):
        ref = R.reference(x, y, t, fair, np.asarray(rp, dtype=np.float64))
        pre = 'fair_' if fair else ''
        for weighted, ww in ((False, 1.0), (True, w)):
            nm = lambda a: V._nanmean(a * ww, ax)      # noqa: E731
            got = V.categorical_error(ens, val, t, pre + 'rps', axis=axis, weighted=weighted)
            assert got.dtype == np.float64
            _close(got, nm(ref['rps']))
            got = V.categorical_error(ens, val, t, pre + 'rpss', axis=axis, weighted=weighted, probabilities=rp)
            _close(got, 1 - nm(ref['rps']) / nm(ref['rps_ref']))
            if not fair:
                got = V.categorical_error(ens, val, t, 'brier', axis=axis, weighted=weighted)
                assert got.shape == nm(ref['rps']).shape + (Q,)
                for j in range(Q):
                    _close(got[..., j], nm(ref['brier'][j]))
    if axis is None:
        assert V.categorical_error(ens, val, t).shape == (SHAPE[0],)          # 'rps', the forecast hour kept


def test_rps_with_one_threshold_is_the_brier_score():
    rng = np.random.default_rng(5)
    x, y, t = _ensemble(rng, q=1)
    assert np.array_equal(V.ranked_probability_score(x, y, t), V.brier_score(x, y, t)[0], equal_nan=True)
    a, b = V.categorical_error(x, y, t, 'rps'), V.categorical_error(x, y, t, 'brier')
    assert np.array_equal(a, b[..., 0])
    # and the skill score of one threshold is the Brier skill score
    bss = 1 - b[..., 0] / V._nanmean(np.where(np.isnan(V.brier_score(x, y, t)[0]), np.nan,
                                              (0.5 - (y <= t[0])) ** 2), (1, 2, 3, 4))
    _close(V.categorical_error(x, y, t, 'rpss', probabilities=(0.5,)), bss, 1e-12)


def test_rpss_of_the_reference_forecast_is_zero():
    """an ensemble whose members split exactly like the reference probabilities: k = (1, 3) of 4 members under the two
    thresholds issues (0.25, 0.75) everywhere, so rps equals rps_ref element by element and the skill is exactly 0"""
    rng = np.random.default_rng(6)
    shape = (2, 7, 3)
    x = rng.permuted(np.tile(np.array([1., 2., 2.5, 4.], dtype=F)[:, None], (1, 42)), axis=0).reshape((4,) + shape)
    t = np.array([1.5, 3.], dtype=F)
    y = rng.choice(np.array([0., 2., 5.], dtype=F), shape)
    assert set(np.unique(V.ensemble_probability(x, t)[0])) == {0.25} and set(np.unique(V.ensemble_probability(x, t)[1])) == {0.75}
    got = V.categorical_error(x, y, t, 'rpss', probabilities=(0.25, 0.75))
    assert got.shape == (2,) and (got == 0.0).all()
    assert (V.categorical_error(x, y, t, 'rpss', probabilities=(0.25, 0.75), axis=(0, 1, 2)) == 0.0).all()


def test_reliability_counts():
    rng = np.random.default_rng(7)
    x, y, t = _ensemble(rng)
    ref = R.reference(x, y, t)
    code = ref['code']
    full = V.reliability_counts(x, y, t)
    assert full.dtype == np.int64 and full.shape == (Q, M + 1, 2)
    for j in range(Q):
        n_ok = int((code[j] >= 0).sum())
        assert full[j].sum() == n_ok == y.size - int(np.isnan(ref['brier'][j]).sum())        # the non-missing elements
        for k in range(M + 1):
            for o in range(2):
                assert full[j, k, o] == int((code[j] == 2 * k + o).sum())
    ens, val = _labelled(x, ('member',) + DIMS), _labelled(y, DIMS)
    thr = Forecast(t, ('quantile',) + DIMS, dict(val.coords, quantile=np.array([0.3, 0.6])))
    part = V.reliability_counts(ens, val, thr, axis=(1, 2, 3))
    assert part.dims == ('f_hour', 'varlev', 'threshold', 'members_below', 'observed') and part.values.shape == (3, 2, Q, M + 1, 2)
    assert np.array_equal(part.coords['threshold'], [0.3, 0.6]) and np.array_equal(part.coords['members_below'], np.arange(M + 1))
    assert np.array_equal(part.coords['observed'], [0, 1]) and np.array_equal(part.values.sum(axis=(0, 1)), full)
    for f in range(3):
        for v in range(2):
            c = code[:, f, :, :, :, v]
            assert part.values[f, v, 1, 2, 1] == int((c[1] == 5).sum())
    # the curves the docstring derives: observed frequency per forecast probability, and one ROC point
    c = full[0].astype(np.float64)
    k_of, o_of = code[0][code[0] >= 0] // 2, code[0][code[0] >= 0] % 2
    assert np.allclose(c[2, 1] / c[2].sum(), o_of[k_of == 2].mean())
    assert np.allclose(c[3:, 1].sum() / c[:, 1].sum(), (k_of[o_of == 1] >= 3).mean())
    assert np.allclose(c[3:, 0].sum() / c[:, 0].sum(), (k_of[o_of == 0] >= 3).mean())


def test_known_values():
    x = np.array([1., 2., 3., 4.], dtype=F).reshape(4, 1)
    y = np.array([2.], dtype=F)
    assert V.ensemble_probability(x, [1.5, 4.5])[:, 0].tolist() == [0.25, 1.0]
    assert V.brier_score(x, y, [1.5, 4.5])[:, 0].tolist() == [0.0625, 0.0]
    assert V.ranked_probability_score(x, y, [1.5, 4.5])[0] == 0.0625
    assert V.brier_score(x, y, [1.5, 3.5])[:, 0].tolist() == [0.0625, 0.0625]         # k = (1, 3), o = (0, 1)
    assert abs(V.ranked_probability_score(x, y, [1.5, 4.5], fair=True)[0] - (0.0625 - 3.0 / 48.0)) < 1e-15
    assert V.reliability_counts(x, y, [1.5, 4.5])[:, :, :].nonzero()[1].tolist() == [1, 4]
    one = np.array([[3.]], dtype=F)                                                  # one member: a deterministic forecast
    assert V.brier_score(one, np.array([2.], dtype=F), [2.5])[0, 0] == 1.0 and V.ensemble_probability(one, [3.])[0, 0] == 1.0


def test_refusals():
    rng = np.random.default_rng(8)
    x, y, t = _ensemble(rng, holes=False)
    with pytest.raises(NotImplementedError, match='lagged'):
        V.brier_score(x, y[0], t)                                      # a continuous series: one axis fewer
    with pytest.raises(NotImplementedError, match='lagged'):
        V.categorical_error(x, y[0], t)
    with pytest.raises(NotImplementedError, match='lagged'):
        V.reliability_counts(x, y[0], t)
    with pytest.raises(ValueError):
        V.ranked_probability_score(x, y[:, :2], t)                     # neither 1 nor the extent
    with pytest.raises(ValueError, match='thresholds'):
        V.brier_score(x, y, t[:, :, :2])
    with pytest.raises(ValueError, match='thresholds'):
        V.brier_score(x, y, t[:, 0])                                   # neither a vector nor the element dims
    with pytest.raises(ValueError, match='method'):
        V.categorical_error(x, y, t, 'crps')
    with pytest.raises(ValueError, match='probabilities'):
        V.categorical_error(x, y, t, 'rpss')
    with pytest.raises(ValueError, match='probabilities'):
        V.categorical_error(x, y, t, 'fair_rpss', probabilities=(0.5,))
    with pytest.raises(ValueError, match='probabilities'):
        V.categorical_error(x, y, t, 'rpss', probabilities=(0.5, 1.5))
    with pytest.raises(ValueError, match='at least 2'):
        V.ranked_probability_score(x[:1], y, t, fair=True)
    with pytest.raises(ValueError, match='at least 2'):
        V.categorical_error(x[:1], y, t, 'fair_rps')
    with pytest.raises(ValueError):
        V.brier_score(x, y, t, member_axis=9)
    with pytest.raises(ValueError, match='threshold_axis'):
        V.brier_score(x, y, t, threshold_axis=9)
    ens, val = _labelled(x, ('member',) + DIMS), _labelled(y, DIMS)
    val.coords['lat'] = val.coords['lat'] + 0.5
    with pytest.raises(ValueError, match='lat'):
        V.categorical_error(ens, val, t)
    assert V._ENS_METHODS == ('crps', 'fair_crps', 'spread', 'ens_mse', 'ens_rmse', 'ssr')          # left alone


def test_device_path_refusals_answered_on_the_host():
    import torch
    from DLWP import _native as nat
    from DLWP import ops
    assert (ops.CATEGORY_MAX_M, ops.CATEGORY_MAX_Q) == (R.MAX_M, R.MAX_Q) == (1024, 16)
    assert ops.ensemble_category_plan((1024, 8), (8, 1), (16,), (1,))['q_class'] == 16
    with pytest.raises(NotImplementedError, match='1024'):
        ops.ensemble_category_plan((1025, 8), (8, 1), (2,), (1,))
    with pytest.raises(NotImplementedError, match='16'):
        ops.ensemble_category_plan((4, 8), (8, 1), (17,), (1,))
    with pytest.raises(ValueError, match='aligned'):
        ops.ensemble_category_plan((4, 8), (8, 1), (2,), (1,), thr_ptr=(1 << 22) + 2)
    with pytest.raises(nat.NativeError):
        ops.ensemble_category(torch.zeros(4, 8), None, torch.zeros(2))              # no CPU fallback behind the device entry
    # unit dims are dropped and adjacent dims merged: one merged dim for contiguous operands
    lay = ops.category_layout((3, 1, 5, 1, 8), (40, 40, 8, 8, 1), (2, 1, 5, 1, 8), (40, 40, 8, 8, 1), 0, 0, (1, 5, 1, 8), (40, 8, 8, 1))
    assert lay[:4] == (3, 40, 2, 40) and lay[6] == [(40, (1, 1, 1))]
    import ctypes
    d = ops.category_desc(4, 8, 2, 8, [(8, (1, 1, 1))])
    lib = nat.lib()
    assert lib.dlwpcs_ensemble_category(ctypes.byref(d), 256, None, 512, 1024, 2048, None, None, None, None) == -1
    assert b'need a verification' in lib.dlwpcs_last_error()
    assert lib.dlwpcs_ensemble_category(ctypes.byref(d), 256, 768, 512, None, None, None, None, None, None) == -1
    assert b'no output' in lib.dlwpcs_last_error()
