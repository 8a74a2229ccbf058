"""
Forecast scores on the device (dlwpcs_score, DLWP/verify.py device path) and the estimator's device-resident forecast and
verification.  Against the reference's golden values (tests/golden/g13_scores.npz), an fp64 restatement (also at 3e8 terms per
output), the host path, contiguous copies of strided views, and itself (bitwise, run to run).
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, 'golden'))
import gen_golden_scores as gs   # noqa: E402

pytestmark = pytest.mark.gpu


class DevLat(object):
    """a device tensor with `.lat` (numpy's trailing-axis rule: no `.dims`)"""
    def __init__(self, values, lat):
        self.values, self.lat = values, lat

    @property
    def shape(self):
        return tuple(self.values.shape)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to('cuda:0')


def _device_fns():
    from DLWP import verify

    def up(x):
        if isinstance(x, gs.WithLat):
            return DevLat(_dev(np.asarray(x)), x.lat)
        return _dev(x) if isinstance(x, np.ndarray) else x

    def fe(f, v, **kw):
        if kw.get('climatology') is not None:
            kw['climatology'] = up(kw['climatology'])
        return verify.forecast_error(up(f), up(v), **kw)

    def pe(p, v, n, **kw):
        return verify.persistence_error(up(p), up(v), n, **kw)

    def ce(v, n, **kw):
        return verify.climo_error(up(v), n, **kw)
    return fe, pe, ce


def _close(got, want, rtol, atol):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    np.testing.assert_allclose(got[ok], want[ok], rtol=rtol, atol=atol)


def _fp64_fns():
    """the host path on fp64 copies of the inputs: the fp64 restatement"""
    from DLWP import verify

    def f64(x):
        if isinstance(x, gs.WithLat):
            return gs.WithLat(np.asarray(x, np.float64), x.lat)
        return np.asarray(x, np.float64) if isinstance(x, np.ndarray) else x

    def fe(f, v, **kw):
        if kw.get('climatology') is not None:
            kw['climatology'] = f64(kw['climatology'])
        return verify.forecast_error(f64(f), f64(v), **kw)
    return (fe, lambda p, v, n, **kw: verify.persistence_error(f64(p), f64(v), n, **kw),
            lambda v, n, **kw: verify.climo_error(f64(v), n, **kw))


def test_device_path_matches_golden_and_fp64(golden_dir):
    g = np.load(os.path.join(golden_dir, 'g13_scores.npz'))
    table = json.loads(str(g['cases']))
    d = {k: g[k] for k in g.files if not k.startswith('case')}
    dev, f64 = _device_fns(), _fp64_fns()
    for i, c in enumerate(table):
        want = g[gs.case_key(i, c)]
        got = gs.run_case(dev, d, c)
        acc = c['method'] == 'acc'
        _close(got, want, 1e-5, 1e-5 if acc else 0.)
        _close(got, gs.run_case(f64, d, c), 1e-6, 1e-6 if acc else 0.)


def test_repeated_calls_are_bitwise_equal_and_views_match_copies():
    from DLWP.verify import forecast_error
    rng = np.random.default_rng(7)
    base = _dev(rng.standard_normal((5, 7, 6, 8, 8, 4)).astype(np.float32))
    v = _dev(rng.standard_normal((5, 7, 6, 8, 8, 4)).astype(np.float32))
    clim = _dev(rng.standard_normal((6, 8, 8, 4)).astype(np.float32))
    perm = base.permute(1, 0, 2, 3, 4, 5).contiguous().permute(1, 0, 2, 3, 4, 5)     # strided view, same values
    assert not perm.is_contiguous()
    for method, kw in (('rmse', {}), ('mae', {}), ('acc', {'climatology': clim})):
        for axis in (None, (1, 2, 3, 4), 1):
            a = forecast_error(base, v, method=method, axis=axis, **kw)
            b = forecast_error(base, v, method=method, axis=axis, **kw)
            assert np.array_equal(a, b, equal_nan=True)
            c = forecast_error(perm, v, method=method, axis=axis, **kw)
            _close(c, a, 1e-6, 1e-6)
    # transposed verification and a broadcast (expanded) climatology
    vt = v.transpose(2, 5).contiguous().transpose(2, 5)
    ce = clim.expand(5, 7, 6, 8, 8, 4)
    a = forecast_error(base, v, 'acc', axis=(1, 2, 3, 4), climatology=clim)
    b = forecast_error(base, vt, 'acc', axis=(1, 2, 3, 4), climatology=ce)
    _close(b, a, 1e-6, 1e-6)


def test_nan_counts_are_per_term():
    """acc: each of the three means skips its own NaNs (a NaN forecast removes a term from two of them, not three)"""
    from DLWP.verify import forecast_error
    rng = np.random.default_rng(8)
    f = rng.standard_normal((2, 9, 40)).astype(np.float32)
    v = rng.standard_normal((2, 9, 40)).astype(np.float32)
    f[rng.random(f.shape) < 0.3] = np.nan
    v[rng.random(v.shape) < 0.2] = np.nan
    for axis in (None, 1, (1, 2)):
        host = forecast_error(f.astype(np.float64), v.astype(np.float64), 'acc', axis=axis, climatology=0.1)
        dev = forecast_error(_dev(f), _dev(v), 'acc', axis=axis, climatology=0.1)
        _close(dev, host, 1e-6, 1e-6)
        _close(forecast_error(_dev(f), _dev(v), 'mse', axis=axis), forecast_error(f.astype(np.float64), v.astype(np.float64),
                                                                                   'mse', axis=axis), 1e-6, 0.)


@pytest.mark.parametrize('method', ['mse', 'acc'])
def test_accuracy_at_3e8_terms_per_output(method):
    n = 300_000_000
    g = torch.Generator(device='cuda:0').manual_seed(11)
    f = torch.randn((1, 1000, n // 1000), device='cuda:0', generator=g)
    v = f * 0.8 + 0.3 * torch.randn((1, 1000, n // 1000), device='cuda:0', generator=g) + 0.5
    from DLWP.verify import forecast_error
    kw = {'climatology': 0.25} if method == 'acc' else {}
    got = forecast_error(f, v, method, **kw)
    fd, vd = f.double(), v.double()
    if method == 'mse':
        want = ((vd - fd) ** 2).mean().item()
    else:
        av, af = vd - 0.25, fd - 0.25
        want = ((av * af).mean() / torch.sqrt((av * av).mean() * (af * af).mean())).item()
    del fd, vd
    rel = abs(got[0] - want) / abs(want)
    print('%s at 3e8 terms: %.3g relative' % (method, rel))
    assert rel <= 1e-6


def test_estimator_device_forecast_and_verification():
    from DLWP.keras import backend
    backend.set_device('cuda:0')
    from DLWP.model import DLWPFunctional, TimeSeriesEstimator
    from DLWP.model.cs_unet import build_cs_model
    from DLWP.model.generators import ArrayDataGenerator
    from DLWP.verify import forecast_error
    N, V, K, T, ITS, n_out = 16, 4, 2, 40, 2, 2
    rng = np.random.default_rng(77)
    arr = rng.standard_normal((T, V, 6, N, N)).astype(np.float32)
    sol = rng.random((T, 6, N, N)).astype(np.float32)
    const = rng.standard_normal((K, 6, N, N)).astype(np.float32)
    lat = rng.uniform(-89, 89, (6, N, N))
    dlwp = DLWPFunctional(is_convolutional=True, time_dim=ITS)
    kw = dict(rank=3, batch_size=2, input_time_steps=ITS, output_time_steps=ITS, sequence=n_out, insolation_array=sol,
              constants=const, channels_last=True)
    gen = ArrayDataGenerator(dlwp, arr, device=True, **kw)
    np.random.seed(3)
    model = build_cs_model(gen.convolution_shape, ITS * V, 'unet2', base_filter_number=8, integration_steps=n_out,
                           io_time_steps=ITS, insolation_shape=gen.insolation_shape, constants_shape=(6, N, N, K))
    dlwp.build_model(model, loss='mse', optimizer='adam')
    times = np.arange('2000-01-01T00', T * 6, 6, dtype='datetime64[h]').astype('datetime64[ns]')
    lon = rng.uniform(0, 360, (6, N, N))
    est = TimeSeriesEstimator(dlwp, gen, sample_times=times, lat=lat, lon=lon)   # insolation computed past the data's end
    samples = np.array([2, 7, 34])                                                # the last one runs past the data: NaN
    steps = 12
    fc = est.predict(steps, samples=samples)
    fd = est.predict(steps, samples=samples, keep_on_device=True)
    assert isinstance(fd.values, torch.Tensor) and fd.values.is_cuda and fd.values.dtype == torch.float32
    assert fd.dims == fc.dims and all(np.array_equal(fd.coords[k], fc.coords[k]) for k in fc.dims)
    est.predict(steps, samples=[0, 1, 3], keep_on_device=True)                  # a later rollout must not overwrite fd
    assert np.array_equal(fd.values.cpu().numpy(), fc.values) and np.array_equal(np.asarray(fd), fc.values)
    vh = est.verification(steps, samples=samples)
    vd = est.verification(steps, samples=samples, keep_on_device=True)
    assert isinstance(vd.values, torch.Tensor) and vd.values.is_cuda
    assert np.array_equal(vd.values.cpu().numpy(), vh.values, equal_nan=True) and np.isnan(vh.values).any()
    clim = rng.standard_normal((6, N, N, V)).astype(np.float32)
    for method, kw2 in (('rmse', {}), ('mae', {}), ('acc', {'climatology': clim}), ('acc', {'climatology': _dev(clim)})):
        dev = forecast_error(fd, vd, method, axis=(1, 2, 3, 4), weighted=True, **kw2)
        host = forecast_error(fc, vh, method, axis=(1, 2, 3, 4), weighted=True, **kw2)
        assert dev.shape == (steps, V)
        _close(dev, host, 1e-6, 1e-6)


def _labelled(x, dims):
    from DLWP.model.extensions import Forecast
    return Forecast(x, dims, {d: np.arange(n) for d, n in zip(dims, x.shape)})


@pytest.mark.parametrize('axis', [(2, 3), (1, 2, 3, 4), (1,)])
def test_cos_on_labelled_device_forecast_matches_fp64(axis):
    from DLWP.verify import forecast_error
    rng = np.random.default_rng(21)
    f = rng.standard_normal((3, 20, 6, 16, 16, 4)).astype(np.float32)
    v = (0.6 * f + rng.standard_normal(f.shape)).astype(np.float32)
    c = (0.2 * rng.standard_normal((6, 16, 16, 4))).astype(np.float32)
    dims = ['f_hour', 'time', 'x0', 'x1', 'x2', 'varlev']
    got = forecast_error(_labelled(_dev(f), dims), _labelled(_dev(v), dims), 'cos', axis=axis, climatology=_dev(c))
    want = forecast_error(_labelled(f.astype(np.float64), dims), _labelled(v.astype(np.float64), dims), 'cos', axis=axis,
                          climatology=c.astype(np.float64))
    _close(got, want, 1e-6, 1e-6)


@pytest.mark.parametrize('method', ['rmse', 'mae', 'acc'])
def test_two_channel_per_variable_scores_match_fp64(method):
    """a kept channel axis of extent 2 (handled inside the workgroup, two float4 slots per channel)"""
    from DLWP.verify import forecast_error
    rng = np.random.default_rng(22)
    f = rng.standard_normal((4, 30, 6, 16, 16, 2)).astype(np.float32)
    v = rng.standard_normal((4, 30, 6, 16, 16, 2)).astype(np.float32)
    v[rng.random(v.shape) < 0.05] = np.nan
    c = rng.standard_normal((6, 16, 16, 2)).astype(np.float32)
    kw = {'climatology': c} if method == 'acc' else {}
    got = forecast_error(_dev(f), _dev(v), method, axis=(1, 2, 3, 4), **kw)
    kw64 = {'climatology': c.astype(np.float64)} if method == 'acc' else {}
    want = forecast_error(f.astype(np.float64), v.astype(np.float64), method, axis=(1, 2, 3, 4), **kw64)
    assert got.shape == (4, 2)
    _close(got, want, 1e-6, 1e-6)


def test_many_short_reductions_match_fp64():
    """~2e6 outputs of 4 terms (axis=-1) and 1.5e5 outputs of 30 (axis=1): one lane per output"""
    from DLWP.verify import climo_error, forecast_error
    rng = np.random.default_rng(23)
    f = rng.standard_normal((8, 30, 6, 32, 32, 4)).astype(np.float32)
    v = rng.standard_normal((8, 30, 6, 32, 32, 4)).astype(np.float32)
    v[rng.random(v.shape) < 0.05] = np.nan
    f64, v64 = f.astype(np.float64), v.astype(np.float64)
    for method in ('mse', 'acc'):
        kw = {'climatology': 0.1} if method == 'acc' else {}
        for axis in (-1, 1):
            got = forecast_error(_dev(f), _dev(v), method, axis=axis, **kw)
            _close(got, forecast_error(f64, v64, method, axis=axis, **kw), 1e-6, 1e-6)
    _close(climo_error(_dev(v[0]), 3, 'rmse', axis=0), climo_error(v64[0], 3, 'rmse', axis=0), 1e-6, 0.)


def test_series_shorter_than_the_forecast():
    """forecast[f, :V - f] against valid[f:] when the forecast has more times than the series (also persistence)"""
    from DLWP.verify import forecast_error, persistence_error
    rng = np.random.default_rng(24)
    f = rng.standard_normal((3, 40, 6, 8, 8, 4)).astype(np.float32)
    v = rng.standard_normal((30, 6, 8, 8, 4)).astype(np.float32)
    for axis in (None, 0, (0, 1, 2, 3)):
        _close(forecast_error(_dev(f), _dev(v), 'rmse', axis=axis), forecast_error(f.astype(np.float64), v.astype(np.float64),
                                                                                  'rmse', axis=axis), 1e-6, 0.)
    with pytest.warns(DeprecationWarning):
        got = persistence_error(_dev(f[0]), _dev(v), 4, 'mae')
    with pytest.warns(DeprecationWarning):
        want = persistence_error(f[0].astype(np.float64), v.astype(np.float64), 4, 'mae')
    _close(got, want, 1e-6, 0.)


_LAUNCH_SCRIPT = r'''
import sys
sys.path[:0] = [%r, %r]
import numpy as np, torch
from DLWP.verify import forecast_error, climo_error
from DLWP.model.extensions import Forecast
f = torch.randn(4, 50, 6, 8, 8, 4, device='cuda:0')
v = torch.randn(4, 50, 6, 8, 8, 4, device='cuda:0')
dims = ['f_hour', 'time', 'x0', 'x1', 'x2', 'varlev']
co = {d: np.arange(s) for d, s in zip(dims, f.shape)}
fv, vv = Forecast(f, dims, co), Forecast(v, dims, co)
vv.lat = Forecast(np.linspace(-80, 80, 6 * 64).reshape(6, 8, 8), dims[2:5], {d: co[d] for d in dims[2:5]})
mark = torch.zeros(8, device='cuda:0')
calls = [lambda: forecast_error(fv, vv, 'rmse', axis=(1, 2, 3, 4), weighted=True),
         lambda: forecast_error(f, v, 'acc', climatology=np.zeros((6, 8, 8, 4), np.float32)),
         lambda: climo_error(v[0], 3, 'mse'),
         lambda: forecast_error(f, v[0], 'mse')]
for call in calls:
    torch.cuda.synchronize()
    torch.cumsum(mark, 0)                   # marker launch between the calls
    torch.cuda.synchronize()
    call()
torch.cuda.synchronize()
torch.cumsum(mark, 0)
torch.cuda.synchronize()
'''


def test_kernel_trace_shows_at_most_three_launches_per_call():
    """four calls in a fresh process under rocprofv3 --kernel-trace --stats: at most 3 dlwpcs_score launches each, and nothing
    else but the runtime's copies (host weights / climatology up, the score table down)"""
    exe = shutil.which('rocprofv3') or ('/opt/rocm/bin/rocprofv3' if os.path.exists('/opt/rocm/bin/rocprofv3') else None)
    if exe is None:
        pytest.skip('rocprofv3 not installed')
    with tempfile.TemporaryDirectory() as tmp:
        script = os.path.join(tmp, 'calls.py')
        open(script, 'w').write(_LAUNCH_SCRIPT % (ROOT, os.path.join(ROOT, 'dlwp-cs_amd')))
        r = subprocess.run(['timeout', '-k', '10', '300', exe, '--kernel-trace', '--stats', '-d', tmp, '-o', 'run',
                            '--output-format', 'csv', '--', sys.executable, script], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        traces = [os.path.join(dp, fn) for dp, _, fns in os.walk(tmp) for fn in fns if fn.endswith('kernel_trace.csv')]
        assert traces, os.listdir(tmp)
        import csv
        rows = []
        for t in traces:
            with open(t) as fh:
                rows += list(csv.DictReader(fh))
        names = [row['Kernel_Name'] for row in sorted(rows, key=lambda r: int(r['Start_Timestamp']))]
    marks = [i for i, n in enumerate(names) if 'scan' in n.lower() or 'cumsum' in n.lower()]
    assert len(marks) >= 5, names
    # the marker may take more than one launch: a call's launches are the non-marker ones between two marker groups
    groups, cur = [], None
    for i, n in enumerate(names[marks[0]:], marks[0]):
        if i in marks:
            if cur:
                groups.append(cur)
            cur = []
        elif cur is not None:
            cur.append(n)
    assert len(groups) == 4, (groups, names)
    for g in groups:
        mine = [n for n in g if 'score_' in n]
        # the rest are the runtime's copy blits: the upload of host weights / climatology and the one download of the result
        copies = [n for n in g if 'score_' not in n]
        assert 1 <= len(mine) <= 3, g
        assert all(n.startswith('__amd_rocclr_copy') for n in copies) and len(copies) <= 2, g
    print('kernel trace: score launches per call %s' % [sum('score_' in n for n in g) for g in groups])
