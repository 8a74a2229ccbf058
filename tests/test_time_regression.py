"""
The least-squares fits of DLWP.verify on the host: harmonic_basis, time_regression, regression_fitted, regression_residual,
detrend and harmonic_climatology on numpy and labelled inputs against the reference of time_regression_ref.py -- values, dims,
coordinates, the missing-value rules and the refusals; the ctypes rows and the planner through the C ABI.  No device.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import time_regression_ref as R     # noqa: E402

from DLWP import verify                             # noqa: E402
from DLWP.model.extensions import Forecast          # noqa: E402


def _series(T=200, shape=(3, 4), seed=0, holes=0.1):
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(T,) + shape) * 5. + 270.).astype(np.float32)
    x[rng.random(x.shape) < holes] = np.nan
    times = np.datetime64('2001-01-01T00') + np.arange(T) * np.timedelta64(6, 'h')
    return x, times


def _close(coef, want):
    """the host path against the reference: the same operations but numpy's summation order -- half an ulp of the final rounding
    on each side and the fp64 solve error, the bound of test_time_regression_ref.py"""
    assert coef.dtype == np.float32 and np.array_equal(np.isnan(coef), np.isnan(want))
    scale = np.max(np.where(np.isnan(want), 0., np.abs(want)), axis=0, keepdims=True)
    ok = ~np.isnan(want)
    assert ok.any() and np.all((np.abs(coef.astype(np.float64) - want) <= 2 * R.U * scale)[ok])


def test_harmonic_basis():
    times = np.datetime64('2001-01-01T00') + np.arange(4 * 1461) * np.timedelta64(6, 'h')      # four years of 365.25 days
    b = verify.harmonic_basis(times, n_harmonics=3, trend=True)
    assert b.dtype == np.float64 and b.shape == (len(times), 8)
    assert np.all(b[:, 0] == 1.) and b[0, 1] == -1. and b[-1, 1] == 1. and abs(b[:, 1].mean()) < 1e-12
    assert np.all(np.diff(b[:, 1]) > 0)
    # harmonics of the tropical year, phase counted from 2000-01-01
    sec = (times - np.datetime64('2000-01-01T00')) / np.timedelta64(1, 's')
    for h in (1, 2, 3):
        ang = 2. * np.pi * h * sec / (365.24219 * 86400.)
        assert np.allclose(b[:, 2 * h], np.cos(ang), atol=1e-9) and np.allclose(b[:, 2 * h + 1], np.sin(ang), atol=1e-9)
    # numbers need a period; over whole periods the harmonics are orthogonal to each other and to the mean
    with pytest.raises(ValueError):
        verify.harmonic_basis(np.arange(10.))
    t = np.arange(3 * 360)
    b = verify.harmonic_basis(t, n_harmonics=4, period=360)
    G = b.T @ b
    want = np.diag([len(t)] + [len(t) / 2.] * 8)
    assert b.shape == (len(t), 9) and np.all(np.abs(G - want) < 1e-9)
    assert verify.harmonic_basis(t, 0, period=5.).shape == (len(t), 1)
    assert verify.harmonic_basis(t, 7, trend=True, period=5.).shape == (len(t), 16)
    with pytest.raises(ValueError):
        verify.harmonic_basis(t, 8, period=5.)                      # 17 terms
    with pytest.raises(ValueError):
        verify.harmonic_basis(t, 2, period=0.)
    with pytest.raises(ValueError):
        verify.harmonic_basis(t.reshape(2, -1), 2, period=5.)


@pytest.mark.parametrize('K', (1, 2, 5, 10, 16))
def test_time_regression_host_against_the_reference(K):
    x, times = _series(seed=K)
    T = x.shape[0]
    b = R.harmonic_basis(T, K).astype(np.float64) * (1. + 2.0 ** -30)          # not float32 values: rounded once, to the reference's
    b32 = b.astype(np.float32)
    for missing, mode in (('skip', R.SKIP), ('propagate', R.PROPAGATE)):
        for mc in (None, T - 25):
            want, n, _ = R.fit_ref(x.reshape(T, -1), b32, mode, mc)
            coef, cnt = verify.time_regression(x, b, missing=missing, min_count=mc, return_count=True)
            assert coef.shape == (K, 3, 4) and cnt.shape == (3, 4) and cnt.dtype == np.int32
            assert np.array_equal(cnt.reshape(-1), n)
            if mode == R.PROPAGATE:
                assert np.isnan(coef).all() and np.isnan(want).all()
            else:
                _close(coef.reshape(K, -1), want)
    xc = np.nan_to_num(x, nan=270.)
    want = R.fit_ref(xc.reshape(T, -1), b32, R.PROPAGATE)[0]
    _close(verify.time_regression(xc, b, missing='propagate').reshape(K, -1), want)
    # another axis
    coef = verify.time_regression(np.moveaxis(xc, 0, 1), b, axis=1, missing='propagate')
    assert coef.shape == (3, K, 4)
    _close(np.moveaxis(coef, 1, 0).reshape(K, -1), want)


def test_fitted_residual_and_detrend_against_the_reference():
    x, times = _series(seed=3)
    T = x.shape[0]
    b = R.harmonic_basis(T, 6)
    coef = verify.time_regression(x, b)
    fit = verify.regression_fitted(coef, b)
    res = verify.regression_residual(x, coef, b)
    assert np.array_equal(np.isnan(fit), np.isnan(R.apply_ref(b, coef.reshape(6, -1)).reshape(fit.shape)))
    assert np.all(np.abs(fit.reshape(T, -1) - R.apply_ref(b, coef.reshape(6, -1))) <= 2 * R.U * 512)
    want = R.apply_ref(b, coef.reshape(6, -1), x.reshape(T, -1))
    assert res.shape == x.shape and np.array_equal(np.isnan(res.reshape(T, -1)), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.all(np.abs(res.reshape(T, -1) - want)[ok] <= 2.0 ** -16)
    # a basis of another length
    b2 = R.harmonic_basis(17, 6, period=T / 2.3)
    fit2 = verify.regression_fitted(coef, b2)
    assert fit2.shape == (17, 3, 4) and np.all(np.abs(fit2.reshape(17, -1) - R.apply_ref(b2, coef.reshape(6, -1))) <= 2 * R.U * 512)
    # detrend: powers of the centred row number
    t = (2. * np.arange(T) - (T - 1)) / (T - 1)
    for order in range(4):
        bp = np.stack([t ** p for p in range(order + 1)], axis=1).astype(np.float32)
        cw = R.fit_ref(x.reshape(T, -1), bp)[0]
        want = R.apply_ref(bp, cw, x.reshape(T, -1))
        got = verify.detrend(x, order=order)
        assert got.shape == x.shape and got.dtype == np.float32 and np.array_equal(np.isnan(got.reshape(T, -1)), np.isnan(want))
        assert np.all(np.abs(got.reshape(T, -1) - want)[~np.isnan(want)] <= 2.0 ** -12)
        assert abs(np.nanmean(got)) < 1e-3
    assert np.isnan(verify.detrend(x, missing='propagate')).all()
    with pytest.raises(ValueError):
        verify.detrend(x, order=4)


def test_labels_kept():
    x, times = _series(T=1461, shape=(2, 5), seed=5)
    ds = Forecast(np.moveaxis(x, 0, 1), ('varlev', 'time', 'cell'), {'varlev': np.array(['z500', 't2m']), 'time': times, 'cell': np.arange(5)})
    ds.lat = np.linspace(-60, 60, 5)
    b = verify.harmonic_basis(times, 2)
    coef, cnt = verify.time_regression(ds, b, return_count=True)
    assert coef.dims == ('varlev', 'term', 'cell') and np.array_equal(coef.coords['term'], np.arange(5))
    assert np.array_equal(coef.coords['varlev'], ds.coords['varlev']) and np.array_equal(coef.lat, ds.lat)
    assert cnt.dims == ('varlev', 'cell') and np.array_equal(cnt.values, (~np.isnan(x)).sum(axis=0))
    fit = verify.regression_fitted(coef, b, times=times)
    assert fit.dims == ds.dims and np.array_equal(fit.coords['time'], times)
    res = verify.regression_residual(ds, coef, b)
    assert res.dims == ds.dims and np.array_equal(res.coords['time'], times) and res.values.shape == ds.values.shape
    assert verify.detrend(ds).dims == ds.dims
    assert verify.time_regression(ds, b, axis='time').dims == coef.dims
    # the harmonic climatology: coefficients, the series at other times, anomalies
    hc = verify.harmonic_climatology(ds, n_harmonics=2, trend=True)
    assert hc.coefficients.dims == ('varlev', 'term', 'cell') and hc.coefficients.values.shape == (2, 6, 5)
    valid = times[40:80:4] + np.timedelta64(365, 'D')
    ser = hc.series(valid)
    assert ser.dims == ('varlev', 'time', 'cell') and np.array_equal(ser.coords['time'], valid) and ser.values.shape == (2, 10, 5)
    lag = hc.series(valid, f_hour=[0, 6, 24])
    assert lag.dims == ('f_hour', 'varlev', 'time', 'cell') and lag.values.shape == (3, 2, 10, 5)
    assert np.array_equal(lag.values[0], ser.values) and np.array_equal(lag.coords['f_hour'], [0, 6, 24])
    assert np.array_equal(lag.values[2], hc.series(valid + np.timedelta64(24, 'h')).values)
    an = hc.anomalies(ds)
    assert an.dims == ds.dims and np.array_equal(np.isnan(an.values), np.isnan(ds.values))
    # the series at the data's own times is what the anomalies subtract
    own = hc.series(times)
    ok = ~np.isnan(ds.values)
    assert np.all(np.abs(ds.values - own.values - an.values)[ok] <= 2.0 ** -15)
    # against the reference on the same rounded basis
    b32 = verify.harmonic_basis(times, 2, True).astype(np.float32)
    want = R.fit_ref(x.reshape(1461, -1), b32)[0]
    _close(np.moveaxis(hc.coefficients.values, 1, 0).reshape(6, -1), want)
    # a noisy annual cycle is recovered: the fitted climatology is far closer to the truth than the spread of the data
    assert np.nanstd(an.values) < 6. and abs(np.nanmean(an.values)) < 0.1


def test_refusals():
    x, times = _series(T=30)
    with pytest.raises(ValueError):
        verify.time_regression(x, np.ones((30, 17)))                    # K > 16
    with pytest.raises(ValueError):
        verify.time_regression(x, R.harmonic_basis(30, 4), min_count=3)  # min_count < K
    bad = R.harmonic_basis(30, 4).astype(np.float64)
    bad[2, 2] = np.nan
    with pytest.raises(ValueError):
        verify.time_regression(x, bad)
    bad[2, 2] = 1e300                                                   # finite in float64, not in float32
    with pytest.raises(ValueError):
        verify.time_regression(x, bad)
    with pytest.raises(ValueError):
        verify.time_regression(x, R.harmonic_basis(29, 4))              # the wrong number of rows
    with pytest.raises(ValueError):
        verify.time_regression(x, np.ones(30))
    with pytest.raises(ValueError):
        verify.time_regression(x, R.harmonic_basis(30, 4), missing='drop')
    with pytest.raises(ValueError):
        verify.regression_fitted(np.zeros((3, 4), np.float32), R.harmonic_basis(30, 4))
    with pytest.raises(ValueError):
        verify.harmonic_climatology(x)


def test_ctypes_rows_and_the_planner_through_the_abi():
    from DLWP import _native as nat
    from DLWP import ops
    for name, nargs in (('dlwpcs_time_regression_scratch_bytes', 5), ('dlwpcs_time_regression', 17),
                        ('dlwpcs_time_regression_plan_info', 12), ('dlwpcs_time_regression_apply', 11)):
        res, args = nat.PROTOTYPES[name]
        assert len(args) == nargs and res is (ctypes.c_size_t if name.endswith('bytes') else ctypes.c_int)
    assert nat.PROTOTYPES['dlwpcs_time_regression'][1][7] is ctypes.c_double                # pivot_tol
    assert nat.REGRESSION_MAX_TERMS == R.MAX_TERMS and nat.REGRESSION_SLAB_ROWS == R.SLAB_ROWS
    lib = nat.lib()
    for T, K, E, slab, split, gram in ((1100, 10, 1028, None, None, None), (1100, 8, 1028, None, None, True), (512, 8, 1028, None, None, None),
                                       (40, 3, 5, 8, None, None), (40, 3, 5, 8, False, None), (0, 1, 256, None, None, None),
                                       (20000, 16, 600000, None, None, None), (20000, 4, 400000, None, None, None),
                                       (100, 4, 0, None, None, None), (97, 5, 1028, 10, True, True)):
        p = ops.time_regression_plan((T, E), (E, 1), K, slab_rows=slab, split=split, gram=gram)
        want = R.plan(T, K, E, E % 4 == 0, slab or 0, -1 if split is None else int(split), -1 if gram is None else int(gram))
        assert (int(p['split']), int(p['gram']), p['k_class'], p['chunk'], p['grid'], p['slab_rows']) == want, (T, K, E)
        assert p['lds_bytes'] == 0
        q = ops.time_regression_plan((T, E), (E, 1), K, slab_rows=slab, split=split, gram=gram, aligned=False)
        assert q['chunk'] == 1
    # scratch: the shared factor always, the slab sums where the call may split
    d, _ = ops.rows_layout((1100, 1028), (1028, 1), 0, None, 10)
    fac = int(lib.dlwpcs_time_regression_scratch_bytes(ctypes.byref(d), 1100, 10, 0, 0))
    assert fac == (160 + 3 * 136) * 8 + 1028 * (10 * 8 + 4)         # the factor, the three slab sums of its G, one part of c and n
    assert int(lib.dlwpcs_time_regression_scratch_bytes(ctypes.byref(d), 1100, 10, 0, -1)) == (160 + 3 * 136) * 8 + 3 * 1028 * (10 * 8 + 4)
    assert int(lib.dlwpcs_time_regression_scratch_bytes(ctypes.byref(d), 1100, 10, 100, 1)) == (160 + 11 * 136) * 8 + 11 * 1028 * (10 * 8 + 4)
    # argument errors come back before any launch, with a message
    info = (ctypes.c_int32 * 8)()
    for args in ((1100, 17, 0, 17, 0, -1, -1), (1100, 4, 2, 4, 0, -1, -1), (1100, 4, 0, 3, 0, -1, -1), (1100, 4, 0, 4, -1, -1, -1),
                 (1100, 4, 0, 4, 0, 2, -1), (1100, 4, 0, 4, 0, -1, -2), (-1, 4, 0, 4, 0, -1, -1)):
        T, K, mode, mc, slab, split, gram = args
        assert lib.dlwpcs_time_regression_plan_info(ctypes.byref(d), 1 << 20, 1 << 20, T, K, mode, mc, slab, split, gram, 1028, info) == -1
        assert b'time_regression' in lib.dlwpcs_last_error()
    assert lib.dlwpcs_time_regression(ctypes.byref(d), 1 << 20, 1100, 1 << 20, 4, 0, 4, ctypes.c_double(1.5), 0, -1, -1, 1 << 20, 1028, None,
                                      None, 0, None) == -1
    assert b'pivot_tol' in lib.dlwpcs_last_error()
    assert lib.dlwpcs_time_regression(ctypes.byref(d), 1 << 20, 1100, 1 << 20, 4, 0, 4, ctypes.c_double(0.), 0, -1, -1, 1 << 20, 1028, None,
                                      None, 0, None) == -1
    assert b'scratch' in lib.dlwpcs_last_error()
    assert lib.dlwpcs_time_regression_apply(ctypes.byref(d), None, 10, 1 << 20, 4, 1 << 20, 1028, None, 1, 1 << 20, None) == -1
    assert b'null operand' in lib.dlwpcs_last_error()
    with pytest.raises(nat.NativeError):
        import torch
        ops.time_regression(torch.zeros(8, 4), np.ones((8, 1)))      # no CPU fallback
