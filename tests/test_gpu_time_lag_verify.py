"""
GPU tests of the lagged-covariance functions of DLWP.verify on device tensors against their float64 host path on the AR(1) cases
of tests/time_lag_ref.py (phi = 0.8, standard deviation 100 on an offset of 5500): every element inside the derived bound, the
counts equal, the results on the device and labelled like the host's.

The bound of a covariance is time_lag_ref.bound().  The derived functions are quotients of covariances computed in float32 on
the device; their bounds follow to first order, u = 2^-24 per float32 operation, dX the bound of X:
    autocorrelation   r_l = c_l / c_0                         dr = (dc_l + |r| dc_0) / c_0 + u |r|
    pair correlation  r = c / (sqrt(va) sqrt(vb))             dr = dc / (sa sb) + |r| (dva / (2 va) + dvb / (2 vb) + 4 u)
    biased covariance c n_l / n_0                             dc + 2 u |c|
    regression slope  s = c / vi                              ds = dc / vi + |s| (dvi / vi + u)
    decorrelation     tau = k + (hi - thr) / (hi - lo)        df = (dhi + u (|hi - thr| + thr)) / D + f (dhi + dlo + u D) / D + u f,
                                                              D = hi - lo, f the fraction; dtau = df + u tau
    sample size, ar1  n (1 - r) / (1 + r)                     2 n dr / (1 + r)^2 + 4 u ess
    sample size, sum  n / (1 + 2 S), S = sum (1 - k / n) r_k  dS = sum (1 - k / n) dr_k + (K + 2) u sum |(1 - k / n) r_k|;
                                                              2 ess dS / (1 + 2 S) + 2 u ess
all times (1 + 1e-4) for the second-order terms, which are 1e-5 of the first-order ones here.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import time_lag_ref as R         # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -24
SECOND = 1.0 + 1e-4
T, E = 600, 24
_CASES = {}


def _case(nan):
    """(a, b) float32 AR(1) series (T, E), shared"""
    if nan not in _CASES:
        rng = np.random.default_rng(40 + nan)
        _CASES[nan] = (R.ar1(rng, T, E, nan_fraction=0.01 * nan), R.ar1(rng, T, E, nan_fraction=0.01 * nan))
    return _CASES[nan]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _inside(got, want, lim, what):
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float32, what
    got, want = got.cpu().numpy().astype(np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    lim = np.broadcast_to(lim, want.shape) * SECOND
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), '%s: NaN pattern' % what
    same_inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), same_inf) and np.array_equal(got[same_inf], want[same_inf]), what
    err = np.where(nan | same_inf, 0.0, np.abs(got - want))
    worst = np.where(nan | same_inf, 0.0, err - lim)
    assert np.all(worst <= 0.0), '%s: |error| %.3e against the bound %.3e at %s' % (
        what, err.flat[np.argmax(worst)], lim.flat[np.argmax(worst)], np.unravel_index(np.argmax(worst), want.shape))
    return float(np.max(np.where(lim > 0, err / np.where(lim > 0, lim, 1.0), 0.0)))


def _auto_bound(x, lags):
    """(r, dr, c0, dc0) of the autocorrelation at `lags` (0 first)"""
    c, dc = R.bound(x, None, lags)
    assert lags[0] == 0
    r = c / c[0]
    return r, (dc + np.abs(r) * dc[0]) / c[0] + U * np.abs(r), c, dc


@pytest.mark.parametrize('nan', [0, 1])
def test_covariance_forms(nan):
    from DLWP import verify as V
    a, b = _case(nan)
    ad, bd = _dev(a), _dev(b)
    for second, sd, lags in ((None, None, 20), (b, bd, 8), (b[:, 3].copy(), _dev(b[:, 3].copy()), [-9, -6, -3, 0, 3, 6, 9])):
        lg = np.arange(0, 21) if second is None else (np.arange(-8, 9) if isinstance(lags, int) else np.array(lags))
        exact, lim = R.bound(a, second, lg)
        got, cnt = V.lag_covariance(ad, sd, lags, return_count=True)
        want, wn = V.lag_covariance(a, second, lags, return_count=True)
        assert isinstance(cnt, torch.Tensor) and cnt.dtype == torch.int32 and np.array_equal(cnt.cpu().numpy(), wn)
        assert np.abs(want - exact).max() <= 1e-9 * np.abs(exact).max()
        frac = _inside(got, want, lim, 'lag_covariance')
        print('lag_covariance nan %d: largest fraction of the bound %.3f' % (nan, frac))
        var = R.bound(a, None, [0])[0][0]
        assert (lim <= 1e-5 * var).all()
        if 0 in lg:
            gb = V.lag_covariance(ad, sd, lags, norm='biased')
            ratio = wn / wn[lg.tolist().index(0)].astype(np.float64)
            _inside(gb, V.lag_covariance(a, second, lags, norm='biased'), ratio * (lim + 2 * U * np.abs(exact)), 'biased')
        gp = V.lag_covariance(ad, sd, lags, missing='propagate')
        wp = V.lag_covariance(a, second, lags, missing='propagate')
        _inside(gp, wp, lim, 'propagate')
        assert bool(np.isnan(wp).any()) == bool(nan)


@pytest.mark.parametrize('nan', [0, 1])
def test_correlations(nan):
    from DLWP import verify as V
    a, b = _case(nan)
    ad, bd = _dev(a), _dev(b)
    lags = list(range(0, 13))
    r, dr, _, _ = _auto_bound(a, lags)
    got, cnt = V.autocorrelation(ad, 12, return_count=True)
    want, wn = V.autocorrelation(a, 12, return_count=True)
    assert np.array_equal(cnt.cpu().numpy(), wn)
    _inside(got, want, dr, 'autocorrelation')
    assert np.array_equal(got[0].cpu().numpy(), np.ones(E, np.float32))
    # lag 0 not among the lags: one more call, dropped
    _inside(V.lag_correlation(ad, lags=[3, 4, 5]), V.lag_correlation(a, lags=[3, 4, 5]), dr[3:6], 'lag_correlation without lag 0')
    # the pair form
    lg = np.arange(-6, 7)
    c, dc = R.bound(a, b, lg)
    va, dva = R.bound(a, None, [0])
    vb, dvb = R.bound(b, None, [0])
    rr = c / np.sqrt(va * vb)
    lim = dc / np.sqrt(va * vb) + np.abs(rr) * (dva / (2 * va) + dvb / (2 * vb) + 4 * U)
    _inside(V.lag_correlation(ad, bd, 6), V.lag_correlation(a, b, 6), lim, 'pair correlation')


@pytest.mark.parametrize('nan', [0, 1])
def test_lag_regression(nan):
    from DLWP import verify as V
    a, b = _case(nan)
    idx = np.ascontiguousarray(b[:, 5])
    lg = np.arange(-5, 6)
    # cov(index[t], x[t + l]) is the index form at the lag -l
    c, dc = (v[::-1] for v in R.bound(a, idx, -lg[::-1]))
    vi, dvi = (v[0, 0] for v in R.bound(idx[:, None], None, [0]))
    vx, dvx = R.bound(a, None, [0])
    slope, corr = V.lag_regression(_dev(idx), _dev(a), 5, return_correlation=True)
    ws, wc = V.lag_regression(idx, a, 5, return_correlation=True)
    s = c / vi
    _inside(slope, ws, dc / vi + np.abs(s) * (dvi / vi + U), 'regression slope')
    rr = c / np.sqrt(vi * vx)
    _inside(corr, wc, dc / np.sqrt(vi * vx) + np.abs(rr) * (dvi / (2 * vi) + dvx / (2 * vx) + 4 * U), 'regression correlation')
    # a host index with device data is uploaded
    _inside(V.lag_regression(idx, _dev(a), 5), ws, dc / vi + np.abs(s) * (dvi / vi + U), 'host index')


@pytest.mark.parametrize('nan', [0, 1])
def test_decorrelation_time_and_sample_size(nan):
    from DLWP import verify as V
    a, b = _case(nan)
    ad, bd = _dev(a), _dev(b)
    K = 15
    lags = list(range(0, K + 1))
    r, dr, _, _ = _auto_bound(a, lags)
    thr = float(np.exp(-1.0))
    want = V.decorrelation_time(a, K)
    got = V.decorrelation_time(ad, K)
    below = r[1:] < thr
    k = np.argmax(below, axis=0)
    crossed = below.any(axis=0)
    # the crossing must not hinge on the rounding: every r up to it is further from the threshold than its bound
    upto = np.arange(K)[:, None] <= np.where(crossed, k, K)[None]
    assert (np.where(upto, np.abs(r[1:] - thr) - dr[1:], 1.0) > 0).all()
    cols = np.arange(E)
    hi, lo, dhi, dlo = r[k, cols], r[k + 1, cols], dr[k, cols], dr[k + 1, cols]
    D = hi - lo
    f = (hi - thr) / D
    lim = (dhi + U * (np.abs(hi - thr) + thr)) / D + f * (dhi + dlo + U * D) / D + U * f
    lim = np.where(crossed, lim + U * np.abs(want), 0.0)
    _inside(got, want, lim, 'decorrelation_time')
    assert crossed.all() and np.isinf(V.decorrelation_time(ad, 1).cpu().numpy()).all() and np.isinf(V.decorrelation_time(a, 1)).all()
    # effective sample size, ar1
    n = V.lag_covariance(a, lags=[0], return_count=True)[1][0].astype(np.float64)
    want = V.effective_sample_size(a)
    _inside(V.effective_sample_size(ad), want, 2 * n * dr[1] / (1 + r[1]) ** 2 + 4 * U * want, 'effective_sample_size ar1')
    # sum
    w = 1 - np.arange(1, K + 1)[:, None] / n
    S = (w * r[1:]).sum(axis=0)
    dS = (w * dr[1:]).sum(axis=0) + (K + 2) * U * np.abs(w * r[1:]).sum(axis=0)
    want = V.effective_sample_size(a, method='sum', max_lag=K)
    assert (want > 1).all() and (want < n).all()
    _inside(V.effective_sample_size(ad, method='sum', max_lag=K), want, 2 * want * dS / (1 + 2 * S) + 2 * U * want, 'effective_sample_size sum')
    # the pair: the products of the autocorrelations
    rb, drb, _, _ = _auto_bound(b, [0, 1])
    p, dp = r[1] * rb[1], np.abs(r[1]) * drb[1] + np.abs(rb[1]) * dr[1] + U * np.abs(r[1] * rb[1])
    want = V.effective_sample_size(a, b)
    nb = V.lag_covariance(a, b, [0], return_count=True)[1][0].astype(np.float64)
    _inside(V.effective_sample_size(ad, bd), want, 2 * nb * dp / (1 + p) ** 2 + 4 * U * want, 'effective_sample_size pair')


def test_labels_stay_and_results_stay_on_the_device():
    from DLWP import verify as V
    from DLWP.labelled import Forecast
    a, b = _case(1)
    dims, coords = ('time', 'lat', 'lon'), {'time': np.arange(T) * 6, 'lat': np.array([-30., 0., 30.])}
    fh = Forecast(a.reshape(T, 3, 8), dims, coords, name='z500')
    fd = Forecast(_dev(a).view(T, 3, 8), dims, coords, name='z500')
    idx = np.ascontiguousarray(b[:, 0])
    calls = [lambda f: V.lag_covariance(f, lags=[-2, 0, 2], return_count=True)[0], lambda f: V.lag_covariance(f, lags=3, return_count=True)[1],
             lambda f: V.lag_correlation(f, lags=2), lambda f: V.autocorrelation(f, 4), lambda f: V.lag_regression(idx, f, 2),
             lambda f: V.decorrelation_time(f, 12), lambda f: V.effective_sample_size(f)]
    for call in calls:
        h, d = call(fh), call(fd)
        assert d.dims == h.dims and d.name == h.name and set(d.coords) == set(h.coords)
        for k in h.coords:
            assert np.array_equal(d.coords[k], h.coords[k])
        assert isinstance(d.values, torch.Tensor) and d.values.is_cuda and tuple(d.values.shape) == h.values.shape
        assert np.array_equal(np.isnan(d.values.cpu().numpy()), np.isnan(h.values))
    assert call(fd).dims == ('lat', 'lon')
    # the time axis in the middle, by name
    gh = Forecast(np.ascontiguousarray(np.moveaxis(fh.values, 0, 1)), ('lat', 'time', 'lon'), coords)
    gd = Forecast(_dev(gh.values), ('lat', 'time', 'lon'), coords)
    h, d = V.lag_covariance(gh, lags=[0, 1]), V.lag_covariance(gd, lags=[0, 1])
    assert d.dims == ('lat', 'lag', 'lon') == h.dims
    exact, lim = R.bound(a, None, [0, 1])
    assert (np.abs(np.moveaxis(d.values.cpu().numpy(), 1, 0).reshape(2, E) - np.moveaxis(h.values, 1, 0).reshape(2, E)) <= lim * SECOND).all()


def test_lag_regression_onto_the_first_principal_component():
    """the standard second step after an EOF analysis: 64 fields of 600 grid points, lead-lag maps onto PC 1"""
    from DLWP import verify as V
    rng = np.random.default_rng(64)
    x = R.ar1(rng, 64, 600)
    x += (np.sin(np.arange(64) / 5.0)[:, None] * np.linspace(-150, 150, 600)[None]).astype(np.float32)
    xd = _dev(x)
    eof = V.eof_analysis(xd, 3)
    pc1 = np.asarray(eof.pcs_values[:, 0], dtype=np.float32)                 # the index both paths see
    lg = np.arange(-4, 5)
    slope = V.lag_regression(_dev(pc1), xd, 4)
    want = V.lag_regression(pc1, x, 4)
    c, dc = (v[::-1] for v in R.bound(x, pc1, -lg[::-1]))
    vi, dvi = (v[0, 0] for v in R.bound(pc1[:, None], None, [0]))
    _inside(slope, want, dc / vi + np.abs(c / vi) * (dvi / vi + U), 'regression onto PC 1')
    # lag 0 is the EOF pattern itself up to the estimator's divisor: the same sign and shape
    z = slope[lg.tolist().index(0)].cpu().numpy().astype(np.float64)
    from DLWP.labelled import raw
    e1 = raw(eof.eofs).cpu().numpy().astype(np.float64)[0]
    assert np.corrcoef(z, e1)[0, 1] > 0.999
