"""
GPU tests of DLWP.verify.ranks: the four verify functions on device tensors and device-valued Forecasts against their host path
on the same data.  `time_ranks` (with and without pct) gives the same float32 bits and stays on the device; `kendall_tau` and
`mann_kendall` give the same eight integers, and therefore -- the float64 code above them being one and the same -- the same bits
in every field; `spearman_correlation` stays on the device and agrees with the float64 host value to the float32 arithmetic of
the device's lag-0 correlation.  What DLWP.ops.time_rank returns stays on the device.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rank_ref as R                                                      # noqa: E402
from test_gpu_large_index import poisoned_results                        # noqa: E402,F401  (the fixture is autouse here too)

from DLWP import verify                                                   # noqa: E402
from DLWP.labelled import Forecast                                        # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FIELDS = ('tau', 'S', 'var_S', 'z', 'p', 'n')
# spearman on the device: the ranks are exact; their means are rounded to float32 once, which shifts every deviation of a column
# by the same amount and so enters the covariance only in second order; the lag-0 covariance and the two variances are exact fp64
# sums rounded to float32 once each, and the quotient and the root are float32 operations: fewer than 16 roundings of 2^-24 on a
# value of at most 1
SPEARMAN_TOL = 16 * 2.0 ** -24


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _on_device(r):
    v = r.values if hasattr(r, 'dims') else r
    assert isinstance(v, torch.Tensor) and v.is_cuda, 'the result left the device'
    return v.cpu().numpy()


def _raw(r):
    return np.asarray(getattr(r, 'values', r))


def _same_records(h, d):
    assert type(h) is type(d) and np.array_equal(h.counts, d.counts)
    for k in FIELDS:
        x, y = getattr(h, k), getattr(d, k)
        assert getattr(x, 'dims', None) == getattr(y, 'dims', None) and getattr(x, 'name', None) == getattr(y, 'name', None)
        x, y = _raw(x), _raw(y)
        assert x.dtype == y.dtype and x.shape == y.shape
        assert np.array_equal(x.view(np.uint64 if x.dtype == np.float64 else np.int64), y.view(np.uint64 if y.dtype == np.float64 else np.int64)), k


@pytest.mark.parametrize('missing', ['skip', 'propagate'])
@pytest.mark.parametrize('values', ['ties', 'special'])
def test_tensors_equal_the_host_path(values, missing):
    rng = np.random.default_rng(5)
    T, E = 60, 75
    a, b = R.make(rng, T, E, R.PAIR, values, 'scattered')
    a[:, 0] = np.arange(T)
    b[:, 0] = -np.arange(T)
    v = rng.standard_normal(T).astype(np.float32)
    ad, bd, vd = _dev(a), _dev(b), _dev(v)
    for pct in (False, True):
        got = _on_device(verify.time_ranks(ad, pct=pct, missing=missing))
        assert np.array_equal(R.bits(got), R.bits(verify.time_ranks(a, pct=pct, missing=missing)))
    _same_records(verify.mann_kendall(a, missing=missing), verify.mann_kendall(ad, missing=missing))
    _same_records(verify.kendall_tau(a, b, missing=missing), verify.kendall_tau(ad, bd, missing=missing))
    _same_records(verify.kendall_tau(a, v, missing=missing), verify.kendall_tau(ad, vd, missing=missing))
    _same_records(verify.kendall_tau(a, v, missing=missing), verify.kendall_tau(ad, v, missing=missing))     # a host index is uploaded
    k = verify.kendall_tau(ad, bd)
    assert k.tau[0] == -1.0 and ((k.p >= 0) & (k.p <= 1) | np.isnan(k.p)).all()
    for second, sd in ((b, bd), (v, vd)):
        h = verify.spearman_correlation(a, second, missing=missing)
        d = _on_device(verify.spearman_correlation(ad, sd, missing=missing))
        assert d.dtype == np.float32 and d.shape == h.shape and np.array_equal(np.isnan(d), np.isnan(h))
        err = np.nanmax(np.abs(d.astype(np.float64) - h))
        print('spearman: largest difference %.3g (bound %.3g)' % (err, SPEARMAN_TOL))
        assert err <= SPEARMAN_TOL


def test_forecasts_keep_their_labels_and_the_time_axis_is_found():
    rng = np.random.default_rng(6)
    F, T, C, H = 2, 33, 3, 5
    x = rng.integers(0, 7, (F, T, C, H)).astype(np.float32)
    y = rng.standard_normal((F, T, C, H)).astype(np.float32)
    x[rng.random(x.shape) < 0.03] = np.nan
    dims = ('f_hour', 'time', 'varlev', 'lat')
    coords = {'f_hour': np.array([24, 48]), 'time': np.arange(T) * 24, 'varlev': np.array(['z', 't', 'q']), 'lat': np.linspace(-45, 45, H)}
    fh, gh = Forecast(x, dims, coords, 'fc'), Forecast(y, dims, coords, 'ob')
    fd, gd = Forecast(_dev(x), dims, coords, 'fc'), Forecast(_dev(y), dims, coords, 'ob')
    r = verify.time_ranks(fd)
    assert r.dims == dims and r.name == 'time_ranks' and np.array_equal(R.bits(_on_device(r)), R.bits(verify.time_ranks(fh).values))
    _same_records(verify.mann_kendall(fh), verify.mann_kendall(fd))
    _same_records(verify.kendall_tau(fh, gh), verify.kendall_tau(fd, gd))
    m = verify.mann_kendall(fd)
    assert m.p.dims == ('f_hour', 'varlev', 'lat') and m.p.values.shape == (F, C, H)
    s = verify.spearman_correlation(fd, gd)
    assert s.dims == ('f_hour', 'varlev', 'lat') and s.name == 'spearman_correlation'
    h = verify.spearman_correlation(fh, gh).values
    assert np.nanmax(np.abs(_on_device(s).astype(np.float64) - h)) <= SPEARMAN_TOL
    _same_records(verify.mann_kendall(x, axis=1), verify.mann_kendall(_dev(x), axis=1))


def test_what_the_ops_layer_returns_stays_on_the_device():
    from DLWP import ops
    a = _dev(np.random.default_rng(7).standard_normal((20, 9)).astype(np.float32))
    ra, rb, st = ops.time_rank(a, a.clone(), ranks=True)
    for t, dt in ((ra, torch.float32), (rb, torch.float32), (st, torch.int64)):
        assert t.is_cuda and t.dtype == dt and t.device == a.device
    assert torch.equal(ra, rb) and tuple(st.shape) == (8, 1, 9) and int(st[1].sum()) == 9 * 190
    with pytest.raises(TypeError):
        ops.time_rank(a.double())
    with pytest.raises(ValueError):
        ops.time_rank(a, ranks=False, stats=False)
    with pytest.raises(ValueError):
        ops.time_rank(a, a[:5])
