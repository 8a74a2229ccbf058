"""
GPU tests of DLWP.verify.eof on device values against the host path, on the four-mode series of tests/eof_cases.py: eigenvalues
within Weyl's bound and PCs within the Davis-Kahan angle, both computed from the derived bound of tests/row_gram_ref.py; the
patterns and the reconstruction under the bars of test_gpu_time_regression.py; projection of a second series; what stays on the
device; neither path runs the other.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eof_cases as EC           # noqa: E402
import row_gram_ref as R         # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -24
K = 4


@pytest.fixture(scope='module')
def both():
    from DLWP import verify
    x, _ = EC.four_mode_series()
    w = EC.weights()
    xd = torch.from_numpy(x).to(DEV)
    return x, w, xd, verify.eof_analysis(xd, K, weights=w), verify.eof_analysis(x, K + 1, weights=w)


def _covariance_error_bound(x, w):
    """||dC||_F of the device's covariance matrix against the exact one of the same float32 anomalies, from R.bound"""
    r32, norm = EC.weight_root(w)
    ref = R.reference(x.reshape(x.shape[0], -1), r=r32.reshape(-1))
    return float(np.linalg.norm(R.bound(ref))) / norm / (x.shape[0] - 1)


def test_eigenvalues_within_weyls_bound(both):
    x, w, xd, dev, host = both
    lim = _covariance_error_bound(x, w)
    err = np.abs(dev.eigenvalues - host.eigenvalues[:K])
    print('eigenvalue error', err, 'Weyl bound', lim)
    # (the host twin sums the same float32 anomalies in float64: 1e-12 of the largest eigenvalue covers it)
    assert np.all(err <= lim + 1e-12 * host.eigenvalues[0])
    assert dev.n_valid == host.n_valid == x[0].size
    assert abs(dev.total_variance - host.total_variance) <= np.sqrt(x.shape[0]) * lim + 1e-12 * host.total_variance


def test_pcs_within_the_davis_kahan_angle(both):
    x, w, xd, dev, host = both
    lim = _covariance_error_bound(x, w)
    lam = host.eigenvalues
    assert isinstance(dev.pcs, np.ndarray) and dev.pcs.shape == (x.shape[0], K)
    for k in range(K):
        gap = min(lam[k - 1] - lam[k] if k else np.inf, lam[k] - lam[k + 1])
        assert 2 * lim / gap < 0.1, 'the condition says nothing at mode %d' % k
        u, v = dev.pcs[:, k] / np.linalg.norm(dev.pcs[:, k]), host.pcs[:, k] / np.linalg.norm(host.pcs[:, k])
        sine = np.linalg.norm(u - (u @ v) * v)
        print('mode %d: sine %.3e, Davis-Kahan %.3e' % (k, sine, 2 * lim / gap))
        assert u @ v > 0 and sine <= 2 * lim / gap + 1e-12
    lead = np.argmax(np.abs(dev.pcs), axis=0)
    assert np.all(dev.pcs[lead, np.arange(K)] > 0)


def test_patterns_and_reconstruction_under_the_regression_bars(both):
    from DLWP import verify
    x, w, xd, dev, host = both
    assert dev.eofs.is_cuda and dev.eofs.dtype == torch.float32 and tuple(dev.eofs.shape) == (K,) + x.shape[1:]
    assert dev.mean.is_cuda and dev.mean.dtype == torch.float32
    # the patterns are the regression maps on the device's own PCs: the host fit on that basis, under the bar of the coefficients
    basis = np.concatenate([np.ones((x.shape[0], 1)), dev.pcs], axis=1)
    coef = verify.time_regression(x, basis, axis=0, missing='propagate')
    assert np.abs(coef).max() < 300.0
    assert np.all(np.abs(dev.eofs.cpu().numpy() - coef[1:]) <= 4 * U * 300.0)
    assert np.all(np.abs(dev.mean.cpu().numpy() - coef[0]) <= 4 * U * 300.0)
    # the reconstruction of the device's coefficients, under the bar of the fitted values
    rec = dev.reconstruct()
    assert rec.is_cuda and rec.dtype == torch.float32 and tuple(rec.shape) == x.shape
    mine = np.concatenate([dev.mean.cpu().numpy()[None], dev.eofs.cpu().numpy()], axis=0)
    want = verify.regression_fitted(mine, basis, term_axis=0)
    assert np.all(np.abs(rec.cpu().numpy() - want) <= 8 * U * 300.0)
    assert np.abs(rec.cpu().numpy() - x).max() < 20 * EC.NOISE                 # four modes leave the noise
    two = dev.reconstruct(2)
    assert two.is_cuda and np.abs(two.cpu().numpy() - x).max() > 1.0


def test_projection_of_a_second_series(both):
    x, w, xd, dev, host = both
    y, _ = EC.four_mode_series(seed=9, n_rows=21)
    y[:, 2, 3] = np.nan                                        # a hole the analysis did not have: the column drops out
    p = dev.project(torch.from_numpy(y).to(DEV))
    assert isinstance(p, np.ndarray) and p.shape == (21, K) and p.dtype == np.float64
    r32, _ = EC.weight_root(w)
    e = dev.eofs.cpu().numpy().reshape(K, -1)
    ref = R.reference(y.reshape(21, -1), e, r=r32.reshape(-1), given_a=dev.mean.cpu().numpy().reshape(-1), center_b=False)
    norm = float((r32.astype(np.float64).reshape(-1) ** 2)[ref['kept']].sum())
    assert ref['n_valid'] == y[0].size - 1
    want = ref['G'] / norm / dev.eigenvalues[None, :]
    lim = R.bound(ref) / norm / dev.eigenvalues[None, :]
    assert np.all(np.abs(p - want) <= lim + 1e-12 * np.abs(want))
    # and the analysed series comes back as its PCs (bound: test_eof.py)
    Y = R.anomalies(x.reshape(x.shape[0], -1), r=r32.reshape(-1))[0].astype(np.float64)
    lam = dev.eigenvalues
    norm = float((r32.astype(np.float64) ** 2).sum())
    chain = R.bound(R.reference(x.reshape(x.shape[0], -1), e, r=r32.reshape(-1), given_a=dev.mean.cpu().numpy().reshape(-1),
                                center_b=False)) / norm
    # three parts: the patterns' float32 error (test_eof.py), the chains of this product, and the device's PCs being the
    # eigenvectors of its own covariance matrix, ||dC|| away: C p - C_dev p = dC p with |p| = sqrt(T - 1)
    lim = (np.sqrt((Y ** 2).sum(axis=1) / norm)[:, None] * 8 * U * np.sqrt(lam[0]) + chain
           + _covariance_error_bound(x, w) * np.sqrt(x.shape[0] - 1.0)) / lam[None, :]
    assert np.all(np.abs(dev.project(xd) - dev.pcs) <= lim)


def test_pattern_covariance_and_labels_on_the_device(both):
    from DLWP import verify
    x, w, xd, dev, host = both
    C, n = verify.pattern_covariance(xd, weights=w, return_count=True)
    assert C.is_cuda and C.dtype == torch.float64 and int(n) == x[0].size
    Ch = verify.pattern_covariance(x, weights=w)
    r32, norm = EC.weight_root(w)
    lim = R.bound(R.reference(x.reshape(x.shape[0], -1), r=r32.reshape(-1))) / norm / (x.shape[0] - 1)
    assert np.all(np.abs(C.cpu().numpy() - Ch) <= lim + 1e-12 * np.abs(Ch).max())
    X = verify.pattern_covariance(xd, xd[:5] * 0.5, weights=w)
    Xh = verify.pattern_covariance(x, x[:5] * np.float32(0.5), weights=w)
    refx = R.reference(x.reshape(x.shape[0], -1), (x[:5] * np.float32(0.5)).reshape(5, -1), r=r32.reshape(-1))
    assert tuple(X.shape) == (x.shape[0], 5)
    assert np.all(np.abs(X.cpu().numpy() - Xh) <= R.bound(refx) / norm / (x.shape[0] - 1) + 1e-12 * np.abs(Xh).max())
    time = np.arange(x.shape[0]) * 6
    f = verify.Forecast(xd, ('time', 'lat', 'lon'), {'time': time, 'lat': EC.latitudes(), 'lon': np.arange(EC.NLON) * 18.0})
    a = verify.eof_analysis(f, 2, weights=w)
    assert a.eofs.dims == ('mode', 'lat', 'lon') and a.eofs.values.is_cuda and a.pcs.dims == ('time', 'mode')
    assert a.mean.dims == ('lat', 'lon') and a.reconstruct().dims == ('time', 'lat', 'lon')
    assert np.array_equal(a.eigenvalues, dev.eigenvalues[:2])


def test_neither_path_runs_the_other(both, monkeypatch):
    from DLWP import ops, verify
    from DLWP.verify import eof, timeseries
    x, w, xd, dev, host = both

    def boom(*a, **k):
        raise AssertionError('the other path ran')
    monkeypatch.setattr(eof, '_gram_host', boom)
    monkeypatch.setattr(timeseries, '_time_regression_host', boom)
    a = verify.eof_analysis(xd, 2, weights=w)
    a.project(xd[:3])
    a.reconstruct()
    verify.pattern_covariance(xd[:4])
    monkeypatch.undo()
    monkeypatch.setattr(ops, 'row_gram', boom)
    monkeypatch.setattr(ops, 'time_regression', boom)
    monkeypatch.setattr(ops, 'time_regression_apply', boom)
    h = verify.eof_analysis(x, 2, weights=w)
    h.project(x[:3])
    h.reconstruct()
