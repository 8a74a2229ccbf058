"""
Climatologies on the device (dlwpcs_group_mean, dlwpcs_rows_gather, dlwpcs_score_indexed; DLWP/verify.py device path) against
tests/golden/g15_climatology.npz, fp64 numpy at a size that exercises the slab split and both load paths, the host path, and
themselves (bitwise: run to run, split against unsplit, indexed against materialised).

The accuracy bound of a group mean is derived, not tuned: against the fp64 expectation m of n non-NaN members,
|r - m| <= 2**-24 |m| + n 2**-52 mean|x| -- one rounding to fp32 plus the worst case of an fp64 running sum.
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
sys.path.insert(0, HERE)
import test_climatology as tc   # noqa: E402

pytestmark = pytest.mark.gpu

g = tc.g


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to('cuda:0')


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


# ---- the fixture through the device path ---------------------------------------------------------------------------- #

@pytest.mark.parametrize('layout', ['channels_last', 'channels_first', 'time_inside'])
@pytest.mark.parametrize('by', ['dayofyear', 'month'])
def test_device_daily_climatology_matches_golden(g, layout, by):
    from DLWP.verify import daily_climatology
    data, times = g['data'], g['times']
    keys, uniq, want = (g['doy'], g['doy_keys'], g['doy_mean']) if by == 'dayofyear' else (g['month'], g['month_keys'],
                                                                                              g['month_mean'])
    perm = {'channels_last': (0, 1, 2, 3, 4), 'channels_first': (0, 4, 1, 2, 3), 'time_inside': (1, 2, 0, 3, 4)}[layout]
    src = tc.labelled(_dev(data.transpose(perm)), times, tuple(tc.DIMS[p] for p in perm))
    out = daily_climatology(src, by=by)
    assert out.values.is_cuda and out.values.is_contiguous() and out.dims == tuple(by if d == 'time' else d for d in src.dims)
    assert np.array_equal(out.coords[by], uniq)
    tc.check_group_mean(out.values.cpu().numpy().transpose(np.argsort(perm)), want, data, keys, uniq)
    # a channels-first source viewed channels-last (the permuted view is reduced through its strides)
    if layout == 'channels_first':
        view = tc.labelled(src.values.permute(0, 2, 3, 4, 1), times)
        again = daily_climatology(view, by=by)
        tc.check_group_mean(again.values.cpu().numpy(), want, data, keys, uniq)


@pytest.mark.parametrize('lead', ['none', 'int', 'timedelta'])
def test_device_climo_time_series_and_row_gather_are_exact(g, lead):
    from DLWP import ops
    from DLWP.verify import daily_climatology, daily_climo_time_series
    clim = daily_climatology(tc.labelled(_dev(g['data']), g['times']))
    f_hour = {'none': None, 'int': g['ts_f_hour'], 'timedelta': g['ts_f_hour'].astype('timedelta64[h]')}[lead]
    doy = g['ts_doy_none'] if lead == 'none' else g['ts_doy_lead']
    table = clim.values.cpu().numpy()
    want = table[np.searchsorted(g['doy_keys'], doy)]
    out = daily_climo_time_series(clim, g['ts_times'], f_hour)
    assert out.values.is_cuda and tuple(out.values.shape) == want.shape
    assert np.array_equal(out.values.cpu().numpy().view(np.int32), want.view(np.int32))
    # negative indices give NaN rows; a strided and a permuted source
    idx = np.array([3, -1, 0, len(table) - 1, -7, 3])
    ref = np.where((idx < 0).reshape(-1, 1, 1, 1, 1), np.nan, table[np.maximum(idx, 0)]).astype(np.float32)
    got = ops.rows_gather(clim.values, idx)
    assert np.array_equal(got.cpu().numpy(), ref, equal_nan=True)
    wide = torch.zeros((len(table), 7) + table.shape[1:], device='cuda:0')
    wide[:, 2] = clim.values
    assert np.array_equal(ops.rows_gather(wide[:, 2], idx).cpu().numpy(), ref, equal_nan=True)
    got = ops.rows_gather(clim.values, _dev(idx.astype(np.int32)), out_perm=(0, 4, 1, 2, 3))
    assert got.is_contiguous() and np.array_equal(got.cpu().numpy(), ref.transpose(0, 4, 1, 2, 3), equal_nan=True)


def test_device_monthly_climo_error_matches_golden(g):
    cases = json.loads(str(g['cases']))
    for c in cases:
        got = tc.run_monthly_case(g, c, wrap=_dev)
        print('monthly_climo_error %s: device %r golden %r' % ({k: c[k] for k in ('method', 'by_day_of_year', 'weighted',
                                                                                 'climo_da')}, got, c['value']))
        tc.check_monthly(got, c)
    from DLWP.verify import monthly_climo_error
    da = tc.labelled(_dev(g['data']), g['times'], lat=g['lat'])
    me, anomaly = monthly_climo_error(da, g['val_set'], method='mae', by_day_of_year=True, return_da=True)
    want = g['anomaly_dayofyear_own']
    assert anomaly.values.is_cuda and np.array_equal(np.isnan(anomaly.values.cpu().numpy()), np.isnan(want))
    atol = 2. ** -23 * float(np.abs(g['data'][np.isfinite(g['data'])]).max())
    np.testing.assert_allclose(anomaly.values.cpu().numpy(), want, rtol=0., atol=atol, equal_nan=True)
    with pytest.raises(KeyError, match='2004-07-04'):
        monthly_climo_error(da, np.concatenate([g['val_set'][:3], g['missing_time']]))


# ---- the kernel at size ----------------------------------------------------------------------------------------------- #

def _big(T, inner, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((T,) + inner) * 5. + 250.).astype(np.float32)
    x[..., -1] = (rng.standard_normal((T,) + inner[:-1]) * 1e-3).astype(np.float32)         # cancels: |m| << mean|x|
    x[rng.random(x.shape) < 0.003] = np.nan
    x[5::7, 0, 1] = np.nan
    x[11, 1, 2] = np.inf
    x[12, 1, 3] = -np.inf
    return x


def _keys(T, K, seed):
    rng = np.random.default_rng(seed)
    if K == 1:
        return np.zeros(T, np.int64)
    k = rng.integers(0, K, T)
    k[:K] = np.arange(K)
    return k


def _expect(x, keys, K):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        with np.errstate(invalid='ignore'):
            return np.stack([np.nanmean(x[keys == k].astype(np.float64), axis=0) for k in range(K)])


def _csr(keys, K):
    order = np.argsort(keys, kind='stable')
    return np.concatenate([[0], np.cumsum(np.bincount(keys, minlength=K))]), order


@pytest.mark.parametrize('K', [366, 12, 1])
@pytest.mark.parametrize('inner', [(6, 40), (5, 37)])                      # 16-byte loads; inner size not a multiple of 4
def test_group_mean_at_size_split_and_unsplit_are_bitwise_equal(K, inner):
    from DLWP import ops
    T = 3300
    x, keys = _big(T, inner, 21), _keys(T, K, 22)
    x[keys == 0, 0, 2] = np.nan                                             # an element whose group holds only NaN
    start, order = _csr(keys, K)
    want = _expect(x, keys, K)
    xd = _dev(x)
    outs = {}
    for split in (None, False, True):
        a, n = ops.group_mean(xd, start, order, split=split, counts=True)
        b = ops.group_mean(xd, start, order, split=split)
        assert np.array_equal(_bits(a), _bits(b)), 'two calls differ (split=%s)' % split
        outs[split] = a
        cnt = np.stack([(~np.isnan(x[keys == k])).sum(axis=0) for k in range(K)])
        assert n.dtype == torch.int32 and np.array_equal(n.cpu().numpy(), cnt)
    assert np.array_equal(_bits(outs[False]), _bits(outs[True])), 'the slab split changes the bits'
    assert np.array_equal(_bits(outs[None]), _bits(outs[True]))
    tc.check_group_mean(outs[True].cpu().numpy(), want, x, keys, np.arange(K))
    # a permuted view (the contiguous axis is not the last), a non-contiguous row stride, an unaligned base, a subset of the rows
    perm = _dev(x.transpose(0, 2, 1)).permute(0, 2, 1)
    assert not perm.is_contiguous() and np.array_equal(_bits(ops.group_mean(perm, start, order)), _bits(outs[True]))
    got = ops.group_mean(xd, start, order, out_perm=(0, 2, 1))
    assert got.is_contiguous() and np.array_equal(_bits(got), _bits(outs[True].permute(0, 2, 1).contiguous()))
    wide = torch.full((T, 3) + inner, 7., device='cuda:0')
    wide[:, 1] = xd
    assert np.array_equal(_bits(ops.group_mean(wide[:, 1], start, order, split=True)), _bits(outs[True]))
    flat = torch.zeros(xd.numel() + 1, device='cuda:0')
    flat[1:] = xd.reshape(-1)
    assert np.array_equal(_bits(ops.group_mean(flat[1:].view(xd.shape), start, order)), _bits(outs[True]))
    some = np.sort(np.random.default_rng(23).choice(T, T // 2, replace=False))
    s2, o2 = _csr(keys[some], K)
    if (np.diff(s2) > 0).all():
        tc.check_group_mean(ops.group_mean(xd, s2, some[o2]).cpu().numpy(), _expect(x[some], keys[some], K), x[some],
                            keys[some], np.arange(K))


def test_group_mean_refuses_a_bad_grouping():
    from DLWP import ops
    x = torch.zeros(8, 4, device='cuda:0')
    with pytest.raises(IndexError):
        ops.group_mean(x, [0, 2], [0, 8])
    with pytest.raises(ValueError):
        ops.group_mean(x, [0, 3], [0, 1])
    with pytest.raises(IndexError):
        ops.rows_gather(x, [0, 8])
    empty, n = ops.group_mean(x, [0, 0, 2], [1, 2], counts=True)
    assert torch.isnan(empty[0]).all() and (n[0] == 0).all() and (empty[1] == 0).all()


# ---- the indexed score -------------------------------------------------------------------------------------------------- #

@pytest.mark.parametrize('method', ['acc', 'cos', 'mse', 'rmse', 'mae'])
@pytest.mark.parametrize('inner', [(6, 8, 8, 4), (6, 8, 8, 2), (3, 5, 7, 3)])
def test_score_indexed_is_bitwise_score_on_the_materialised_operand(method, inner):
    """ops level: the same descriptor with the table looked up and with the gathered (F, T, ...) operand; per-variable (kc = 4, 2
    on the vector path; 3 channels on the scalar path) and reduced over everything (slabs: the two-launch form)"""
    from DLWP import ops
    F, T, K = 5, 60, 17
    gen = torch.Generator(device='cuda:0').manual_seed(5)
    f = torch.randn((F, T) + inner, device='cuda:0', generator=gen)
    v = torch.randn((F, T) + inner, device='cuda:0', generator=gen)
    table = 0.3 * torch.randn((K,) + inner, device='cuda:0', generator=gen)
    w = torch.rand(inner[:-1] + (1,), device='cuda:0', generator=gen) + 0.5
    rows = np.random.default_rng(6).integers(0, K, (F, T)).astype(np.int32)
    rows_d = _dev(rows.reshape(-1))
    full = ops.rows_gather(table, rows_d).reshape((F, T) + inner)
    shape = (F, T) + inner
    st = lambda t: tuple(int(s) for s in t.stride())   # noqa: E731
    lead = method in ('acc', 'cos')
    for red in (set(range(1, len(shape))), set(range(1, len(shape) - 1))):
        for wt in (None, (w, (0, 0) + tuple(0 if e == 1 else s for e, s in zip(w.shape, st(w))))):
            tab = (table, (0, 0) + st(table)[1:])
            mat = (full, st(full))
            a = ops.score_reduce(method, [(f, st(f)) if lead else tab, (v, st(v)), tab if lead else None, wt], shape, red,
                                 lagged=(T, 0), indexed=(rows_d, int(table.stride(0))))
            b = ops.score_reduce(method, [(f, st(f)) if lead else mat, (v, st(v)), mat if lead else None, wt], shape, red,
                                 lagged=(T, 0))
            c = ops.score_reduce(method, [(f, st(f)) if lead else mat, (v, st(v)), mat if lead else None, wt], shape, red)
            assert torch.isfinite(b).all()
            assert np.array_equal(a.cpu().numpy().view(np.int64), b.cpu().numpy().view(np.int64))
            if int(np.prod(inner)) % 4 == 0:
                # the aligned form forecast_error uses for an array climatology merges the time axis into the row; with rows of
                # a multiple of 4 elements that is the same order (rows of odd length: forecast_error materialises a lookup)
                assert np.array_equal(a.cpu().numpy().view(np.int64), c.cpu().numpy().view(np.int64))


def test_score_indexed_with_many_elements_per_output_uses_slabs_and_stays_bitwise():
    from DLWP import ops
    F, T, K, inner = 2, 365, 40, (6, 48, 48, 4)
    gen = torch.Generator(device='cuda:0').manual_seed(8)
    f = torch.randn((F, T) + inner, device='cuda:0', generator=gen)
    v = torch.randn((F, T) + inner, device='cuda:0', generator=gen)
    table = 0.3 * torch.randn((K,) + inner, device='cuda:0', generator=gen)
    rows_d = _dev(np.random.default_rng(9).integers(0, K, F * T).astype(np.int32))
    full = ops.rows_gather(table, rows_d).reshape((F, T) + inner)
    st = lambda t: tuple(int(s) for s in t.stride())   # noqa: E731
    shape, red = (F, T) + inner, {1, 2, 3, 4}
    a = ops.score_reduce('acc', [(f, st(f)), (v, st(v)), (table, (0, 0) + st(table)[1:]), None], shape, red, lagged=(T, 0),
                         indexed=(rows_d, int(table.stride(0))))
    b = ops.score_reduce('acc', [(f, st(f)), (v, st(v)), (full, st(full)), None], shape, red)
    assert a.shape == (F, 4) and np.array_equal(a.cpu().numpy().view(np.int64), b.cpu().numpy().view(np.int64))


@pytest.mark.parametrize('inner', [(6, 8, 8, 4), (3, 5, 7, 3)])
@pytest.mark.parametrize('method', ['acc', 'cos'])
def test_forecast_error_with_a_lookup_is_bitwise_the_materialised_series(inner, method):
    from DLWP.model.extensions import Forecast
    from DLWP.verify import daily_climo_time_series, forecast_error
    F, T, K = 4, 30, 9
    gen = torch.Generator(device='cuda:0').manual_seed(12)
    dims = ['f_hour', 'time', 'x0', 'x1', 'x2', 'varlev']
    times = np.datetime64('2004-02-25T00') + np.arange(T) * np.timedelta64(6, 'h')
    co = {'f_hour': np.arange(F) * 12, 'time': times}
    f = Forecast(torch.randn((F, T) + inner, device='cuda:0', generator=gen), dims, co)
    v = Forecast(torch.randn((F, T) + inner, device='cuda:0', generator=gen), dims, co)
    v.lat = Forecast(np.linspace(-80, 80, int(np.prod(inner[:3]))).reshape(inner[:3]), dims[2:5], {})
    days = np.arange(56, 56 + K)
    clim = Forecast(0.3 * torch.randn((K,) + inner, device='cuda:0', generator=gen), ['dayofyear'] + dims[2:], {'dayofyear': days})
    lazy = daily_climo_time_series(clim, times, co['f_hour'], lazy=True)
    full = daily_climo_time_series(clim, times, co['f_hour'])
    for kw in ({}, {'axis': (1, 2, 3, 4), 'weighted': True}, {'axis': (1, 2)}):
        a = forecast_error(f, v, method, climatology=lazy, **kw)
        b = forecast_error(f, v, method, climatology=full, **kw)
        assert a.shape == b.shape and np.isfinite(a).all() and np.array_equal(a.view(np.int64), b.view(np.int64)), kw


# ---- the estimator chain ------------------------------------------------------------------------------------------------ #

def test_estimator_chain_on_a_device_resident_generator_matches_the_host_path():
    from DLWP.keras import backend
    backend.set_device('cuda:0')
    from DLWP.model import DLWPFunctional, TimeSeriesEstimator
    from DLWP.model.cs_unet import build_cs_model
    from DLWP.model.generators import ArrayDataGenerator
    from DLWP.verify import ClimatologyLookup, daily_climo_time_series, forecast_error
    N, V, T, ITS = 8, 4, 160, 2
    rng = np.random.default_rng(41)
    arr = (rng.standard_normal((T, V, 6, N, N)) + 3. * np.sin(np.arange(T) / 9.)[:, None, None, None, None]).astype(np.float32)
    sol = rng.random((T, 6, N, N)).astype(np.float32)
    times = np.datetime64('2003-12-25T00') + np.arange(T) * np.timedelta64(6, 'h')
    lat = rng.uniform(-89, 89, (6, N, N))
    samples = np.arange(0, 100, 3)
    steps = 6

    def chain(device):
        dlwp = DLWPFunctional(is_convolutional=True, time_dim=ITS)
        gen = ArrayDataGenerator(dlwp, arr, rank=3, batch_size=8, input_time_steps=ITS, output_time_steps=ITS,
                                 insolation_array=sol, channels_last=True, device=device)
        np.random.seed(0)
        model = build_cs_model(gen.convolution_shape, ITS * V, 'unet2', base_filter_number=4)
        dlwp.build_model(model, loss='mse', optimizer='adam')
        est = TimeSeriesEstimator(dlwp, gen, sample_times=times, lat=lat)
        keep = bool(device)
        clim = est.climatology(keep_on_device=keep)
        fc = est.predict(steps, samples, keep_on_device=keep)
        ver = est.verification(steps, samples, keep_on_device=keep)
        c = daily_climo_time_series(clim, fc.coords['time'], fc.coords['f_hour'], lazy=True)
        assert isinstance(c, ClimatologyLookup) and tuple(c.shape) == tuple(fc.shape)
        acc = forecast_error(fc, ver, 'acc', axis=(1, 2, 3, 4), weighted=True, climatology=c)
        return est, clim, fc, ver, c, acc

    est, clim, fc, ver, c, acc = chain(True)
    assert clim.values.is_cuda and fc.values.is_cuda and clim.dims == ('dayofyear', 'x0', 'x1', 'x2', 'varlev')
    _, clim_h, fc_h, ver_h, c_h, acc_h = chain(None)
    assert np.array_equal(clim.coords['dayofyear'], clim_h.coords['dayofyear'])
    assert np.array_equal(c.rows, c_h.rows)
    # the climatology: against fp64 numpy under the derived bound (keys from the host function, itself pinned by the fixture)
    cl = arr.transpose(0, 2, 3, 4, 1)
    from DLWP.verify import calendar_keys
    keys = calendar_keys(times)
    uniq = np.unique(keys)
    want = np.stack([cl[keys == k].astype(np.float64).mean(axis=0) for k in uniq])
    tc.check_group_mean(clim.values.cpu().numpy(), want, cl, keys, uniq)
    tc.check_group_mean(clim_h.values, want, cl, keys, uniq)
    # lazy against materialised on the device: bitwise
    full = c.materialize()
    assert full.values.is_cuda and tuple(full.values.shape) == tuple(fc.shape)
    acc_full = forecast_error(fc, ver, 'acc', axis=(1, 2, 3, 4), weighted=True, climatology=full)
    assert acc.shape == (steps, V) and np.array_equal(acc.view(np.int64), acc_full.view(np.int64))
    # against the host path scoring the device's own forecast (the tolerances of tests/test_gpu_verify_scores.py for 'acc')
    fc_host = type(fc)(fc.values.cpu().numpy(), fc.dims, fc.coords)
    host = forecast_error(fc_host, ver_h, 'acc', axis=(1, 2, 3, 4), weighted=True, climatology=c_h)
    ok = ~np.isnan(host)
    assert np.array_equal(np.isnan(acc), np.isnan(host)) and ok.any()
    print('estimator chain acc: device %s host %s' % (acc[ok][:4], host[ok][:4]))
    np.testing.assert_allclose(acc[ok], host[ok], rtol=1e-5, atol=1e-5)


# ---- launches ----------------------------------------------------------------------------------------------------------- #

_LAUNCH_SCRIPT = r'''
import sys
sys.path[:0] = [%r, %r]
import numpy as np, torch
from DLWP import ops
from DLWP.model.extensions import Forecast
from DLWP.verify import daily_climatology, daily_climo_time_series, forecast_error, monthly_climo_error
T, inner = 1500, (6, 8, 8, 4)
x = torch.randn((T,) + inner, device='cuda:0')
times = np.datetime64('2001-01-01T00') + np.arange(T) * np.timedelta64(6, 'h')
dims = ['time', 'x0', 'x1', 'x2', 'varlev']
da = Forecast(x, dims, {'time': times})
clim = daily_climatology(da)
F, B = 4, 50
fd = ['f_hour'] + dims
co = {'f_hour': np.arange(F) * 6, 'time': times[:B]}
f = Forecast(torch.randn((F, B) + inner, device='cuda:0'), fd, co)
v = Forecast(torch.randn((F, B) + inner, device='cuda:0'), fd, co)
lazy = daily_climo_time_series(clim, times[:B], co['f_hour'], lazy=True)
keys = np.zeros(T, np.int64)
mark = torch.zeros(8, device='cuda:0')
calls = [lambda: daily_climatology(da),
         lambda: daily_climatology(da, by='month'),
         lambda: ops.group_mean(x, [0, T], np.arange(T), split=True),
         lambda: daily_climo_time_series(clim, times[:B], co['f_hour']),
         lambda: forecast_error(f, v, 'acc', axis=(1, 2, 3, 4), climatology=lazy),
         lambda: monthly_climo_error(da, times[100:400:2], method='rmse')]
for call in calls:
    torch.cuda.synchronize()
    torch.cumsum(mark, 0)                   # marker launch between the calls
    torch.cuda.synchronize()
    call()
torch.cuda.synchronize()
torch.cumsum(mark, 0)
torch.cuda.synchronize()
'''


def test_kernel_trace_shows_the_launches_of_every_call():
    """six calls in a fresh process under rocprofv3 --kernel-trace --stats: a climatology takes one or two group_mean launches
    (two only in the slab form), a materialised series one gather, a lazy 'acc' at most two score launches and no gather, a
    monthly_climo_error its climatology plus at most two score launches; beside them only the runtime's copies"""
    exe = shutil.which('rocprofv3') or '/opt/rocm/bin/rocprofv3'
    assert os.path.exists(exe), 'rocprofv3 is part of the ROCm installation this suite needs'
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
    assert len(marks) >= 7, names
    groups, cur = [], None
    for i, n in enumerate(names[marks[0]:], marks[0]):
        if i in marks:
            if cur:
                groups.append(cur)
            cur = []
        elif cur is not None:
            cur.append(n)
    assert len(groups) == 6, (groups, names)

    def count(grp, word):
        return sum(word in n for n in grp)
    mine = ('group_mean_kernel', 'group_finish_kernel', 'rows_gather_kernel', 'score_')
    for grp in groups:
        rest = [n for n in grp if not any(w in n for w in mine)]
        assert all(n.startswith('__amd_rocclr_copy') for n in rest), grp
    print('kernel trace: launches per call %s' % [[w for n in grp for w in mine if w in n] for grp in groups])
    doy, month, forced, series, acc, monthly = groups
    assert count(doy, 'group_mean_kernel') == 1 and count(doy, 'group_finish_kernel') == 0
    assert count(month, 'group_mean_kernel') == 1 and count(month, 'group_finish_kernel') <= 1
    assert count(forced, 'group_mean_kernel') == 1 and count(forced, 'group_finish_kernel') == 1
    assert count(series, 'rows_gather_kernel') == 1 and count(series, 'score_') == 0 and count(series, 'group_') == 0
    assert 1 <= count(acc, 'score_') <= 2 and count(acc, 'rows_gather_kernel') == 0 and count(acc, 'group_') == 0
    assert count(monthly, 'group_mean_kernel') + count(monthly, 'group_finish_kernel') <= 2
    assert 1 <= count(monthly, 'score_') <= 2 and count(monthly, 'rows_gather_kernel') == 0
