#!/usr/bin/env python3
"""
Climatologies on the device (DLWP/verify.py -> dlwpcs_group_mean / dlwpcs_rows_gather / dlwpcs_score_indexed): one JSON line.

At T = 14 600 rows (10 years, 6-hourly) x 4 variables x C48, channels-first fp32 (3.2 GB): milliseconds and effective TB/s
(bytes = the array read once + the result written once) of `daily_climatology` by day of the year and by month into the
channels-first and the channels-last layout, forced into the two-launch slab form as well; the box's copy rate measured in the
same process (a device-to-device copy of the same array: bytes read + written); the same reduction composed from torch ops
(`index_add_` of the rows and of a ones column, then a division: fp32 atomics, no NaN skipping) and from numpy on the host
(at --host-rows rows: the full size takes minutes).  Then weighted per-variable 'acc' at F = 40 leads x T = 365 times with
(a) climatology 0., (b) the materialised series, (c) the lazy lookup, and the gather that materialises the series.
Medians of --reps timed calls after a warm-up call, each ending in a synchronising download.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'dlwp-cs_amd')]

import numpy as np   # noqa: E402
import torch         # noqa: E402


def _time(fn, reps):
    def call():
        r = fn()
        r = r if isinstance(r, torch.Tensor) else getattr(r, 'values', r)
        if isinstance(r, torch.Tensor):
            r.reshape(-1)[:1].cpu()                 # the synchronising download
    call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=14600)
    ap.add_argument('--host-rows', type=int, default=1460)
    ap.add_argument('--leads', type=int, default=40)
    ap.add_argument('--inits', type=int, default=365)
    ap.add_argument('--n', type=int, default=48)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--no-host', action='store_true', help='skip the numpy host path')
    a = ap.parse_args()
    from DLWP import ops
    from DLWP.model.extensions import Forecast
    from DLWP.verify import _csr, calendar_keys, daily_climatology, daily_climo_time_series, forecast_error
    T, N, V = a.rows, a.n, 4
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((T, V, 6, N, N), device=dev, generator=gen)
    times = np.datetime64('1990-01-01T00') + np.arange(T) * np.timedelta64(6, 'h')
    cf = Forecast(x, ['time', 'varlev', 'x0', 'x1', 'x2'], {'time': times})
    cl = Forecast(x.permute(0, 2, 3, 4, 1), ['time', 'x0', 'x1', 'x2', 'varlev'], {'time': times})
    row_bytes = V * 6 * N * N * 4
    out = {'rows': T, 'row_bytes': row_bytes, 'array_GB': round(T * row_bytes / 1e9, 3)}

    spare = torch.empty_like(x)
    ms = _time(lambda: spare.copy_(x), a.reps)
    out['copy'] = {'ms': round(ms, 3), 'TBs': round(2 * T * row_bytes / ms / 1e9, 3)}
    del spare

    def entry(ms, K):
        return {'ms': round(ms, 3), 'TBs': round((T + K) * row_bytes / ms / 1e9, 3)}
    for by in ('dayofyear', 'month'):
        K = len(np.unique(calendar_keys(times, by)))
        out['%s_channels_first' % by] = entry(_time(lambda: daily_climatology(cf, by=by), a.reps), K)
        out['%s_channels_last' % by] = entry(_time(lambda: daily_climatology(cl, by=by), a.reps), K)
        uniq, start, order = _csr(calendar_keys(times, by))
        for split in (False, True):
            out['%s_kernel_%s' % (by, 'two_launches' if split else 'one_launch')] = entry(
                _time(lambda: ops.group_mean(x, start, order, split=split), a.reps), K)
        # the same reduction composed from torch ops
        keys = torch.from_numpy(np.searchsorted(uniq, calendar_keys(times, by))).to(dev)
        ones = torch.ones(T, device=dev)

        def composed():
            s = torch.zeros((K,) + tuple(x.shape[1:]), device=dev).index_add_(0, keys, x)
            n = torch.zeros(K, device=dev).index_add_(0, keys, ones)
            return s / n.reshape((K,) + (1,) * (x.dim() - 1))
        out['%s_torch_index_add' % by] = entry(_time(composed, a.reps), K)
        got, ref = daily_climatology(cf, by=by).values, composed()
        out['%s_max_abs_diff_vs_torch' % by] = float((got - ref).abs().max().item())
    out['one_group_kernel'] = entry(_time(lambda: ops.group_mean(x, [0, T], np.arange(T)), a.reps), 1)

    if not a.no_host:
        Th = min(a.host_rows, T)
        xh = x[:Th].cpu().numpy()
        src = Forecast(xh, cf.dims, {'time': times[:Th]})
        t0 = time.perf_counter()
        daily_climatology(src)
        ms = 1e3 * (time.perf_counter() - t0)
        out['host_numpy_dayofyear'] = {'rows': Th, 'ms': round(ms, 1), 'TBs': round(Th * row_bytes / ms / 1e9, 5)}
        del xh, src

    # weighted per-variable 'acc' with the three climatologies
    clim = daily_climatology(cl)
    del x, cf, cl
    torch.cuda.empty_cache()
    F, B = a.leads, a.inits
    shape = (F, B, 6, N, N, V)
    f = torch.randn(shape, device=dev, generator=gen)
    v = torch.randn(shape, device=dev, generator=gen)
    dims = ['f_hour', 'time', 'x0', 'x1', 'x2', 'varlev']
    co = {'f_hour': np.arange(1, F + 1) * 6, 'time': times[1000:1000 + B]}
    fv, vv = Forecast(f, dims, co), Forecast(v, dims, co)
    vv.lat = Forecast(np.linspace(-85, 85, 6 * N * N).reshape(6, N, N), dims[2:5], {})
    nbytes = 2 * f.numel() * 4
    lazy = daily_climo_time_series(clim, co['time'], co['f_hour'], lazy=True)
    ms_g = _time(lambda: daily_climo_time_series(clim, co['time'], co['f_hour']), a.reps)
    full = lazy.materialize()
    out['acc_shape'] = list(shape)
    out['series_gather'] = {'ms': round(ms_g, 3), 'TBs': round(f.numel() * 4 / ms_g / 1e9, 3)}
    zero = torch.zeros((6, N, N, V), device=dev)
    for name, c in (('acc_climatology_zero', zero), ('acc_materialised', full), ('acc_lazy', lazy)):
        ms = _time(lambda: forecast_error(fv, vv, 'acc', axis=(1, 2, 3, 4), weighted=True, climatology=c), a.reps)
        out[name] = {'ms': round(ms, 3), 'TBs': round(nbytes / ms / 1e9, 3)}
    out['acc_materialised_plus_gather_ms'] = round(out['acc_materialised']['ms'] + ms_g, 3)
    r1 = forecast_error(fv, vv, 'acc', axis=(1, 2, 3, 4), weighted=True, climatology=lazy)
    r2 = forecast_error(fv, vv, 'acc', axis=(1, 2, 3, 4), weighted=True, climatology=full)
    out['acc_lazy_bitwise_equal_materialised'] = bool(np.array_equal(r1.view(np.int64), r2.view(np.int64)))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
