"""
Forecast scores (reference DLWP/verify.py:18-164) on the host path, and `TimeSeriesEstimator.verification`.

The numpy restatement of `forecast_error` / `persistence_error` / `climo_error` against golden values the reference's own
function bodies produced (tests/golden/gen_golden_scores.py), each quirk and refusal of the reference, the name-aligned latitude
weights of a channels_last `Forecast`, and the verification series the estimator builds from its generator.  No device work.
"""
import json
import os
import sys
import warnings

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import gen_golden_scores as gs   # noqa: E402


@pytest.fixture(scope='module')
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, 'g13_scores.npz'))
    return g, json.loads(str(g['cases']))


def _engine():
    from DLWP import verify
    return verify.forecast_error, verify.persistence_error, verify.climo_error


def _check(got, want, method):
    got = np.asarray(got)
    assert got.dtype == np.float64
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    atol = 1e-5 if method == 'acc' else 0.
    np.testing.assert_allclose(got[ok], want[ok], rtol=1e-5, atol=atol)


def test_host_path_matches_every_golden_case(golden):
    g, table = golden
    assert len(table) > 200
    d = {k: g[k] for k in g.files if not k.startswith('case')}
    fns = _engine()
    for i, c in enumerate(table):
        want = g[gs.case_key(i, c)]
        got = gs.run_case(fns, d, c)
        _check(got, want, c['method'])


def test_method_assert_and_acc_warning():
    from DLWP.verify import forecast_error
    x = np.ones((2, 3, 4), np.float32)
    with pytest.raises(AssertionError, match="'method' must be one of 'mse', 'mae', 'rmse', 'acc', 'cos'"):
        forecast_error(x, x, method='bias')
    rng = np.random.default_rng(0)
    f, v = rng.standard_normal((2, 3, 4)), rng.standard_normal((2, 3, 4))
    with pytest.warns(UserWarning, match='expect to get a climatology'):
        r = forecast_error(f, v, method='acc')
    want = np.nanmean(v * f, axis=(1, 2)) / np.sqrt(np.nanmean(v ** 2, axis=(1, 2)) * np.nanmean(f ** 2, axis=(1, 2)))
    np.testing.assert_allclose(r, want, rtol=1e-12)


def test_lagged_climatology_with_leading_dim_is_refused():
    from DLWP.verify import forecast_error
    f = np.zeros((2, 5, 3), np.float32)
    v = np.zeros((5, 3), np.float32)
    with pytest.raises(ValueError, match="'climatology' cannot have non-spatial dimensions"):
        forecast_error(f, v, method='acc', climatology=np.zeros((5, 3)))


def test_lagged_without_climatology_computes_the_natural_result():
    """the reference dereferences climatology.shape here (AttributeError for None / 0.); the engine scores"""
    from DLWP.verify import forecast_error
    rng = np.random.default_rng(1)
    f = rng.standard_normal((3, 6, 4)).astype(np.float32)
    v = rng.standard_normal((6, 4)).astype(np.float32)
    r = forecast_error(f, v, method='rmse')
    want = np.array([np.sqrt(np.mean((v[k:] - f[k, :6 - k]) ** 2.)) for k in range(3)])
    np.testing.assert_allclose(r, want, rtol=1e-6)
    assert r.dtype == np.float64 and r.shape == (3,)


def test_lagged_acc_returns_the_first_lead_unweighted():
    from DLWP.verify import forecast_error
    rng = np.random.default_rng(2)
    f = rng.standard_normal((3, 6, 4)).astype(np.float32)
    v = gs.WithLat(rng.standard_normal((6, 4)).astype(np.float32), np.linspace(-60, 60, 4))
    c = np.zeros(4, np.float32)
    r = forecast_error(f, v, method='acc', climatology=c, weighted=True)
    vv = np.asarray(v)
    want = np.mean(vv * f[0]) / np.sqrt(np.mean(vv ** 2) * np.mean(f[0] ** 2))
    assert np.ndim(r) == 0
    np.testing.assert_allclose(r, want, rtol=1e-6)


def test_cos_needs_labelled_inputs_and_lagged_cos_is_refused():
    from DLWP.model.extensions import Forecast
    from DLWP.verify import forecast_error
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 3, 4)).astype(np.float32)
    y = rng.standard_normal((2, 3, 4)).astype(np.float32)
    with pytest.raises(TypeError, match="'cos' method requires"):
        forecast_error(x, y, method='cos', climatology=0.)
    dims = ['f_hour', 'time', 'x']
    co = {'f_hour': np.arange(2), 'time': np.arange(3), 'x': np.arange(4)}
    fx, fy = Forecast(x, dims, co), Forecast(y, dims, co)
    r = forecast_error(fx, fy, method='cos', axis=(1, 2), climatology=0.)
    want = np.sum(x * y, axis=(1, 2)) / (np.linalg.norm(x, axis=(1, 2)) * np.linalg.norm(y, axis=(1, 2)))
    np.testing.assert_allclose(r, want, rtol=1e-6)
    series = Forecast(y[0], dims[1:], {'time': co['time'], 'x': co['x']})
    with pytest.raises(NotImplementedError, match='verify.py:91-94'):
        forecast_error(fx, series, method='cos', climatology=np.zeros(4))


def test_labelled_inputs_must_agree():
    from DLWP.model.extensions import Forecast
    from DLWP.verify import forecast_error
    x = np.zeros((2, 3), np.float32)
    a = Forecast(x, ['f_hour', 'time'], {'f_hour': np.arange(2), 'time': np.arange(3)})
    b = Forecast(x, ['f_hour', 'time'], {'f_hour': np.arange(2), 'time': np.arange(3) + 1})
    c = Forecast(x, ['f_hour', 'sample'], {'f_hour': np.arange(2), 'sample': np.arange(3)})
    with pytest.raises(ValueError, match="coordinate 'time'"):
        forecast_error(a, b)
    with pytest.raises(ValueError, match='dims'):
        forecast_error(a, c)


def test_persistence_and_climo_refusals():
    from DLWP.verify import climo_error, persistence_error
    x = np.zeros((4, 3), np.float32)
    with pytest.warns(DeprecationWarning):
        with pytest.raises(ValueError, match="'method' must be 'mse', 'rmse', or 'mae'"):
            persistence_error(x, x, 2, method='acc')
    with pytest.raises(ValueError, match="'method' must be 'mse', 'rmse', or 'mae'"):
        climo_error(x, 2, method='cos')


def test_climo_scores_unshifted_rows_against_the_nanmean():
    from DLWP.verify import climo_error
    rng = np.random.default_rng(4)
    v = rng.standard_normal((6, 5)).astype(np.float32)
    v[2, 1] = np.nan
    r = climo_error(v, 3, method='mae', axis=0)
    m = np.nanmean(v, axis=0)
    want = np.array([np.nanmean(np.abs(v[:6 - k] - m), axis=0) for k in range(3)])
    np.testing.assert_allclose(r, want, rtol=1e-6)


def test_all_nan_slice_gives_nan():
    from DLWP.verify import forecast_error
    f = np.zeros((2, 3, 4), np.float32)
    v = np.ones((2, 3, 4), np.float32)
    v[:, :, 1] = np.nan
    r = forecast_error(f, v, method='mse', axis=1)
    assert np.isnan(r[:, 1]).all() and np.array_equal(r[:, [0, 2, 3]], np.ones((2, 3)))


def test_named_weights_of_channels_last_forecast_match_numpy_rule():
    """lat with dims (x0, x1, x2) broadcasts by name against a channels_last Forecast; the same data transposed to channels_first
    with a plain ndarray lat (numpy's trailing-axis rule) gives the same scores"""
    from DLWP.model.extensions import Forecast
    from DLWP.verify import forecast_error
    rng = np.random.default_rng(5)
    F_, T_, N_, C_ = 3, 4, 3, 2
    f = rng.standard_normal((F_, T_, 6, N_, N_, C_)).astype(np.float32)
    v = rng.standard_normal((F_, T_, 6, N_, N_, C_)).astype(np.float32)
    lat = rng.uniform(-80, 80, (6, N_, N_))
    dims = ['f_hour', 'time', 'x0', 'x1', 'x2', 'varlev']
    co = dict(zip(dims, [np.arange(F_), np.arange(T_), np.arange(6), np.arange(N_), np.arange(N_), np.arange(C_)]))
    fv, vv = Forecast(f, dims, co), Forecast(v, dims, co)
    vv.lat = Forecast(lat, ['x0', 'x1', 'x2'], {'x0': co['x0'], 'x1': co['x1'], 'x2': co['x2']}, name='lat')
    cf = (0, 1, 5, 2, 3, 4)
    vcf = gs.WithLat(v.transpose(cf), lat)
    for method, kw in (('mse', {}), ('mae', {}), ('acc', {'climatology': np.zeros((6, N_, N_, C_), np.float32)})):
        a = forecast_error(fv, vv, method=method, axis=(1, 2, 3, 4), weighted=True, **kw)
        kwcf = {'climatology': kw['climatology'].transpose(3, 0, 1, 2)} if kw else {}
        b = forecast_error(f.transpose(cf), vcf, method=method, axis=(1, 3, 4, 5), weighted=True, **kwcf)
        np.testing.assert_allclose(a, b, rtol=1e-12)
        assert a.shape == (F_, C_)


# --------------------------------------------------------------------------------------------------------------------- #
# TimeSeriesEstimator.verification
# --------------------------------------------------------------------------------------------------------------------- #

@pytest.fixture
def host_device():
    from DLWP.keras import backend
    prev = backend.device()
    backend.set_device('cpu')
    yield
    backend.set_device(prev)


@pytest.mark.parametrize('n_out', [1, 2])
@pytest.mark.parametrize('steps', [3, 40])
def test_verification_matches_predict_layout_and_data(host_device, n_out, steps):
    import test_estimator as te
    from DLWP.model import DLWPFunctional, TimeSeriesEstimator
    dlwp = DLWPFunctional(is_convolutional=True, time_dim=te.ITS)
    dlwp.build_model(te._StubNet(n_out), loss='mse')
    gen, sol, const = te._generator(dlwp, n_out if n_out > 1 else None)
    times = np.arange('2000-01-01T00', te.T * 6, 6, dtype='datetime64[h]').astype('datetime64[ns]')
    lat = np.random.default_rng(0).uniform(-90, 90, (6, te.N, te.N))
    lon = np.random.default_rng(1).uniform(0, 360, (6, te.N, te.N))
    est = TimeSeriesEstimator(dlwp, gen, sample_times=times, lat=lat, lon=lon)
    samples = [0, 3, 5]
    fc = est.predict(min(steps, 8), samples=samples)
    ver = est.verification(min(steps, 8), samples=samples)
    assert ver.dims == fc.dims and ver.values.shape == fc.values.shape
    for d in fc.dims:
        assert np.array_equal(ver.coords[d], fc.coords[d])
    assert tuple(ver.lat.dims) == ('x0', 'x1', 'x2') and np.array_equal(ver.lat.values, lat)
    # every value is the data row whose sample time is init + f_hour, NaN past the end of the data
    ver = est.verification(steps, samples=samples)
    arr = gen.array
    f_hour = ver.coords['f_hour']
    for i, fh in enumerate(f_hour):
        for j, t0 in enumerate(ver.coords['time']):
            when = t0 + np.timedelta64(int(fh), 'h')
            row = np.nonzero(times == when)[0]
            got = ver.values[i, j]
            if row.size == 0:
                assert np.isnan(got).all()
            else:
                assert np.array_equal(got, np.moveaxis(arr[row[0]], 0, -1))
    if steps == 40:
        assert np.isnan(ver.values[-1]).all()
    td = est.verification(3, samples=samples, f_hour_timedelta_type=True)
    assert np.array_equal(td.coords['f_hour'], est.predict(3, samples=samples, f_hour_timedelta_type=True).coords['f_hour'])
