"""
CPU tests of DLWP.verify.eof on the host path: eigenvalues against the singular values of the weighted anomalies, the
orthogonality of the patterns, projection and reconstruction, the sign rule, labels, an excluded grid point, every error; and the
descriptor checks of dlwpcs_row_gram that need no device.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eof_cases as EC           # noqa: E402
import row_gram_ref as R         # noqa: E402

EPS = 2.0 ** -24
E_INVALID = -1              # DLWPCS_E_INVALID


@pytest.fixture(scope='module')
def series():
    x, pcs = EC.four_mode_series()
    return x, pcs, EC.weights()


@pytest.fixture(scope='module')
def analysis(series):
    from DLWP import verify
    x, _, w = series
    return verify.eof_analysis(x, 5, weights=w)


def _weighted_anomalies(x, w):
    """(T, E) float64: the float32 anomalies of the definition over the root of the sum of the weights applied"""
    r32, norm = EC.weight_root(w)
    ya = R.anomalies(x.reshape(x.shape[0], -1), r=r32.reshape(-1))[0]
    return ya.astype(np.float64) / np.sqrt(norm)


def test_eigenvalues_are_the_squared_singular_values(series, analysis):
    x, pcs, w = series
    s = np.linalg.svd(_weighted_anomalies(x, w), compute_uv=False)
    want = s ** 2 / (x.shape[0] - 1)
    lam = analysis.eigenvalues
    print('eigenvalues', lam)
    assert lam.shape == (5,) and np.all(np.diff(lam) < 0)
    assert np.all(np.abs(lam[:4] - want[:4]) <= 1e-10 * want[:4])
    assert abs(lam[4] - want[4]) <= 1e-10 * want[0]            # (the noise floor: to the accuracy of the largest)
    assert abs(analysis.total_variance - want.sum()) <= 1e-10 * want.sum()
    assert np.allclose(analysis.variance_fraction, lam / analysis.total_variance, rtol=1e-14)
    assert analysis.n_valid == x[0].size
    assert np.allclose(analysis.north_errors(), lam * np.sqrt(2.0 / x.shape[0]), rtol=1e-14)
    # the four built-in modes, a factor of about 4 apart, over a noise floor
    assert np.all(lam[:3] / lam[1:4] > 2.5) and lam[3] / lam[4] > 1e3
    # the PCs are the series' own up to sign: unit variance, and each correlates with the PC it was built from
    p = analysis.pcs
    assert p.shape == (x.shape[0], 5) and p.dtype == np.float64
    assert np.allclose((p ** 2).sum(axis=0) / (x.shape[0] - 1), 1.0, rtol=1e-12)
    corr = np.abs(p[:, :4].T @ pcs) / (x.shape[0] - 1)
    assert np.all(np.diag(corr) > 0.99)


def test_patterns_are_orthogonal_with_the_eigenvalues_as_norms(series, analysis):
    x, _, w = series
    r32, norm = EC.weight_root(w)
    wa = (r32.astype(np.float64) ** 2 / norm).reshape(-1)
    e = np.asarray(analysis.eofs, dtype=np.float64).reshape(5, -1)
    assert analysis.eofs.dtype == np.float32 and analysis.eofs.shape == (5,) + x.shape[1:]
    got = (e * wa[None]) @ e.T
    lam = analysis.eigenvalues
    # The patterns are the least-squares maps on the PCs rounded to float32, stored in float32.  A basis entry off by 2^-24
    # lets mode k leak into map l by 2^-24 sqrt(lam_k) in the weighted norm, at most sqrt(lam_1) for each of the K + 1 terms, and
    # the storage rounds once more: |sum w e_k e_l - lam_k delta_kl| <= (K + 3) 2^-24 sqrt(lam_1) (sqrt(lam_k) + sqrt(lam_l)).
    lim = 8 * EPS * np.sqrt(lam[0]) * (np.sqrt(lam)[:, None] + np.sqrt(lam)[None, :])
    assert np.all(np.abs(got - np.diag(lam)) <= lim)


def test_projecting_the_series_returns_the_pcs(series, analysis):
    x, _, w = series
    lam = analysis.eigenvalues
    p = analysis.project(x)
    assert p.shape == analysis.pcs.shape and p.dtype == np.float64
    # project uses the anomalies y of the analysis itself, so only the patterns' float32 error d e_k enters:
    # |d pc_k[t]| <= |y_t|_w |d e_k|_w / lam_k with |d e_k|_w <= 8 2^-24 sqrt(lam_1) (above) and |y_t|_w^2 = (T - 1) C[t, t]
    Y = _weighted_anomalies(x, w)
    lim = np.sqrt((Y ** 2).sum(axis=1))[:, None] * 8 * EPS * np.sqrt(lam[0]) / lam[None, :]
    print('projection error / bound', (np.abs(p - analysis.pcs) / lim).max())
    assert np.all(np.abs(p - analysis.pcs) <= lim)
    assert np.all(np.abs(analysis.project(x[5:9]) - analysis.pcs[5:9]) <= lim[5:9])


def test_reconstruction_with_all_modes_returns_the_series():
    from DLWP import verify
    x, _ = EC.four_mode_series(seed=2, n_rows=12)
    x[:, 3, 4] = np.nan
    x[7, 0, 0] = np.inf
    a = verify.eof_analysis(x, 11)
    assert a.n_valid == x[0].size - 2
    rec = a.reconstruct()
    assert rec.shape == x.shape and rec.dtype == np.float32
    gone = np.zeros(x.shape[1:], dtype=bool)
    gone[3, 4] = gone[0, 0] = True
    assert np.isnan(rec[:, gone]).all() and np.isnan(np.asarray(a.eofs)[:, gone]).all() and np.isnan(a.mean[gone]).all()
    # T terms interpolate T rows whatever the rounding of the basis; the float32 coefficients and the result round once each
    basis = np.abs(np.concatenate([np.ones((12, 1)), a.pcs], axis=1).astype(np.float32).astype(np.float64))
    coef = np.abs(np.concatenate([a.mean[None], np.asarray(a.eofs)], axis=0).astype(np.float64))
    lim = 2 * EPS * (np.einsum('tk,kij->tij', basis, coef) + np.abs(x))
    assert np.all(np.abs(rec.astype(np.float64) - x)[:, ~gone] <= lim[:, ~gone])
    # fewer modes: further from the series, and the mean alone with none
    r1 = a.reconstruct(1)
    assert np.nanmax(np.abs(r1 - x)[:, ~gone]) > np.nanmax(np.abs(rec - x)[:, ~gone])
    assert np.allclose(a.reconstruct(0)[:, ~gone], np.broadcast_to(a.mean, x.shape)[:, ~gone], rtol=1e-6)


def test_sign_rule_and_order(analysis):
    p = analysis.pcs
    lead = np.argmax(np.abs(p), axis=0)
    assert np.all(p[lead, np.arange(p.shape[1])] > 0)
    assert np.all(np.diff(analysis.eigenvalues) <= 0)


def test_uncentred_analysis_and_unweighted():
    from DLWP import verify
    x, _ = EC.four_mode_series(seed=4)
    a = verify.eof_analysis(x - 280.0, 3, center=False)
    y = (x - 280.0).reshape(x.shape[0], -1).astype(np.float64)
    want = np.linalg.svd(y, compute_uv=False) ** 2 / (x.shape[0] - 1) / y.shape[1]
    assert np.all(np.abs(a.eigenvalues - want[:3]) <= 1e-10 * want[:3])
    assert np.array_equal(a.mean, np.zeros(x.shape[1:], dtype=np.float32))
    assert np.all(np.abs(a.project(x - 280.0) - a.pcs) <= 1e-4)


def test_labels_and_axis_order(series):
    from DLWP import verify
    x, _, w = series
    lat, lon, time = EC.latitudes(), np.arange(EC.NLON) * 18.0, np.arange(x.shape[0]) * 6
    xs = np.ascontiguousarray(np.moveaxis(x, 0, 1))                # (lat, time, lon)
    f = verify.Forecast(xs, ('lat', 'time', 'lon'), {'lat': lat, 'time': time, 'lon': lon})
    a = verify.eof_analysis(f, 3, weights=w)
    plain = verify.eof_analysis(x, 3, weights=w)
    assert np.allclose(a.eigenvalues, plain.eigenvalues, rtol=1e-12)
    assert a.eofs.dims == ('lat', 'mode', 'lon') and a.eofs.shape == (EC.NLAT, 3, EC.NLON)
    assert np.array_equal(a.eofs.coords['mode'], np.arange(3)) and np.array_equal(a.eofs.coords['lat'], lat)
    assert a.pcs.dims == ('time', 'mode') and np.array_equal(a.pcs.coords['time'], time) and a.pcs.shape == (x.shape[0], 3)
    assert a.mean.dims == ('lat', 'lon')
    assert np.allclose(np.moveaxis(np.asarray(a.eofs.values), 1, 0), plain.eofs, rtol=1e-5, atol=1e-5)
    rec = a.reconstruct()
    assert rec.dims == ('lat', 'time', 'lon') and np.array_equal(rec.coords['time'], time)
    p = a.project(f.isel(time=slice(0, 4)))
    assert p.dims == ('time', 'mode') and np.array_equal(p.coords['time'], time[:4])
    assert np.allclose(p.values, a.pcs.values[:4], atol=1e-4)
    assert np.allclose(verify.eof_analysis(xs, 3, weights=w, axis=1).eigenvalues, plain.eigenvalues, rtol=1e-12)


def test_pattern_covariance_on_the_host(series):
    from DLWP import verify
    x, _, w = series
    C, n = verify.pattern_covariance(x, weights=w, return_count=True)
    Y = _weighted_anomalies(x, w)
    assert C.dtype == np.float64 and n == x[0].size and np.allclose(C, Y @ Y.T / (x.shape[0] - 1), rtol=1e-12, atol=1e-9)
    b = x[:5] * 0.5 + 1.0
    X = verify.pattern_covariance(x, b, weights=w, ddof=0)
    Yb = _weighted_anomalies(b, w)
    assert X.shape == (x.shape[0], 5) and np.allclose(X, Y @ Yb.T / x.shape[0], rtol=1e-12, atol=1e-9)
    wn = w.copy()
    wn[2, 3] = np.nan
    assert verify.pattern_covariance(x, weights=wn, return_count=True)[1] == x[0].size - 1


def test_errors(series):
    from DLWP import verify
    x, _, w = series
    T = x.shape[0]
    for bad in (0, 16, -1):
        with pytest.raises(ValueError):
            verify.eof_analysis(x, bad)
    with pytest.raises(ValueError):
        verify.eof_analysis(x[:9], 9)                           # centred: at most T - 1
    assert verify.eof_analysis(x[:9], 9, center=False).eigenvalues.shape == (9,)
    with pytest.raises(ValueError):
        verify.eof_analysis(x[:9], 10, center=False)
    with pytest.raises(NotImplementedError):
        verify.eof_analysis(np.zeros((verify.EOF_MAX_ROWS + 1, 2), dtype=np.float32), 1)
    with pytest.raises(ValueError):
        verify.eof_analysis(x, 2, weights=-w)
    with pytest.raises(ValueError):
        verify.eof_analysis(x, 2, weights=np.zeros_like(w))
    with pytest.raises(ValueError):
        verify.eof_analysis(x, 2, weights=np.ones((3, 3)))
    with pytest.raises(ValueError):
        verify.eof_analysis(x, 2, ddof=T)
    with pytest.raises(ValueError):
        verify.eof_analysis(np.full_like(x, np.nan), 2)         # nothing is kept
    with pytest.raises(ValueError):
        verify.eof_analysis(x, 2, axis=3)
    with pytest.raises(ValueError):
        verify.pattern_covariance(x, x[:, :5])
    a = verify.eof_analysis(x, 2)
    with pytest.raises(ValueError):
        a.project(x[:, :5])
    with pytest.raises(ValueError):
        a.reconstruct(3)


def test_bad_descriptors_are_rejected_without_a_device():
    from DLWP import _native as nat
    from DLWP import ops
    lib = nat.lib()
    info = (ctypes.c_int64 * 8)()
    d, _ = ops.rows_layout((10, 4, 6), (24, 6, 1), 0, None, 1)
    p = 1 << 20
    assert lib.dlwpcs_row_gram_plan_info(ctypes.byref(d), p, 10, None, None, 0, -1, info) == 0
    assert list(info)[:5] == [1, 1, 1, 1, 1]
    assert lib.dlwpcs_row_gram_plan_info(None, p, 10, None, None, 0, -1, info) == E_INVALID
    assert b'null descriptor' in lib.dlwpcs_last_error()
    assert lib.dlwpcs_row_gram_plan_info(ctypes.byref(d), p, 10, None, p, 5, -1, info) == E_INVALID       # b without db
    other, _ = ops.rows_layout((5, 4, 5), (20, 5, 1), 0, None, 1)
    assert lib.dlwpcs_row_gram_plan_info(ctypes.byref(d), p, 10, ctypes.byref(other), p, 5, -1, info) == E_INVALID
    assert b'is not a' in lib.dlwpcs_last_error()
    two, _ = ops.rows_layout((5, 4, 6), (60, 14, 2), 0, None, 1)
    assert two.n_inner == 2
    assert lib.dlwpcs_row_gram_plan_info(ctypes.byref(d), p, 10, ctypes.byref(two), p, 5, -1, info) == E_INVALID
    neg, _ = ops.rows_layout((10, 4, 6), (24, 6, 1), 0, None, 1)
    neg.inner_ext[0] = -3
    assert lib.dlwpcs_row_gram_plan_info(ctypes.byref(neg), p, 10, None, None, 0, -1, info) == E_INVALID
    assert lib.dlwpcs_row_gram_plan_info(ctypes.byref(d), p, -1, None, None, 0, -1, info) == E_INVALID
    assert lib.dlwpcs_row_gram_plan_info(ctypes.byref(d), p, 10, None, None, 0, 2, info) == E_INVALID
    assert lib.dlwpcs_row_gram_plan_info(ctypes.byref(d), None, 10, None, None, 0, -1, info) == E_INVALID
    assert lib.dlwpcs_row_gram_scratch_bytes(ctypes.byref(neg), 10, None, 0, -1) == 0
    assert lib.dlwpcs_row_gram_scratch_bytes(ctypes.byref(d), 10, None, 0, -1) > 0
    # the entry point checks the same before it launches anything
    for desc, rows in ((None, 10), (ctypes.byref(neg), 10), (ctypes.byref(d), -1)):
        assert lib.dlwpcs_row_gram(desc, p, rows, None, None, 0, None, 1, None, 1, None, -1, p, 10, None, None, p, 1 << 30, None) \
            == E_INVALID
    assert lib.dlwpcs_row_gram(ctypes.byref(d), p, 10, ctypes.byref(other), p, 5, None, 1, None, 1, None, -1, p, 5, None, None, p,
                               1 << 30, None) == E_INVALID
    assert lib.dlwpcs_row_gram(ctypes.byref(d), p, 10, None, None, 0, None, 3, None, 1, None, -1, p, 10, None, None, p, 1 << 30,
                               None) == E_INVALID
    assert lib.dlwpcs_row_gram(ctypes.byref(d), p, 10, None, None, 0, None, 1, None, 1, None, -1, p, 10, None, None, p, 16,
                               None) == E_INVALID           # scratch too small
    with pytest.raises(ValueError):
        ops.row_gram_plan((10, 4, 6), (24, 6, 1), split=2)
    plan = ops.row_gram_plan((300, 40000), (40000, 1), n_rows_b=15)
    assert plan == dict(row_tiles_a=3, row_tiles_b=1, tile_pairs=3, slabs=79, groups=5, split=True, vec=True, grid=15)
    assert not ops.row_gram_plan((300, 40000), (40000, 1), aligned=False)['vec']
    assert not ops.row_gram_plan((300, 40000), (1, 300), row_axis=0)['vec']


def test_a_numpy_input_never_reaches_the_device_wrapper(series, monkeypatch):
    from DLWP import ops, verify
    x, _, w = series

    def boom(*a, **k):
        raise AssertionError('the host path launched')
    monkeypatch.setattr(ops, 'row_gram', boom)
    monkeypatch.setattr(ops, 'time_regression', boom)
    a = verify.eof_analysis(x, 2, weights=w)
    a.project(x[:3])
    a.reconstruct()
    verify.pattern_covariance(x[:4])
