#!/usr/bin/env python3
"""
Forecast scores on the device (DLWP/verify.py -> dlwpcs_score): one JSON line.

At F = 40 leads x T = 365 initialisations x C48 (6*48*48) x C = 4 fp32 channels_last: milliseconds, effective TB/s and the
fraction of the HBM roofline (algorithmic bytes: forecast + verification read once) for aligned rmse (axis=None), per-variable
rmse and latitude-weighted per-variable acc.  In the lagged form (forecast[f, t] against a continuous series[f + t]) every lead
reads T - f forecast rows; the series is counted once.  The lagged cases are rmse, per-variable rmse and latitude-weighted
per-variable rmse: the reference's lagged acc scores the first lead only (DLWP/verify.py:87-90).  Also the numpy host path at
the same size, and end to end on a small model: predict(keep_on_device=True) + verification + forecast_error against
predict() + numpy scoring.
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

HBM_TBS = 8.0        # MI355X peak HBM bandwidth


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()                                   # ends with the result's download: synchronised
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--leads', type=int, default=40)
    ap.add_argument('--inits', type=int, default=365)
    ap.add_argument('--n', type=int, default=48)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--no-host', action='store_true', help='skip the numpy host path')
    ap.add_argument('--no-end-to-end', action='store_true', help='skip the end-to-end model case')
    a = ap.parse_args()
    from DLWP.model.extensions import Forecast
    from DLWP.verify import forecast_error
    F, T, N, C = a.leads, a.inits, a.n, 4
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(0)
    shape = (F, T, 6, N, N, C)
    f = torch.randn(shape, device=dev, generator=g)
    v = torch.randn(shape, device=dev, generator=g)
    series = torch.randn((T + F, 6, N, N, C), device=dev, generator=g)
    dims = ['f_hour', 'time', 'x0', 'x1', 'x2', 'varlev']
    co = {d: np.arange(s) for d, s in zip(dims, shape)}
    lat = np.linspace(-85, 85, 6 * N * N).reshape(6, N, N)
    fv, vv = Forecast(f, dims, co), Forecast(v, dims, co)
    vv.lat = Forecast(lat, dims[2:5], {d: co[d] for d in dims[2:5]})
    clim = torch.zeros((6, N, N, C), device=dev)
    out = {'shape': list(shape), 'hbm_peak_TBs': HBM_TBS}
    nbytes = 2 * f.numel() * 4
    cases = {
        'aligned_rmse': lambda: forecast_error(f, v, 'rmse'),
        'aligned_rmse_per_var': lambda: forecast_error(f, v, 'rmse', axis=(1, 2, 3, 4)),
        'aligned_acc_weighted_per_var': lambda: forecast_error(fv, vv, 'acc', axis=(1, 2, 3, 4), weighted=True, climatology=clim),
    }
    for k, fn in cases.items():
        ms = _time(fn, a.reps)
        out[k] = {'ms': round(ms, 3), 'TBs': round(nbytes / ms / 1e9, 3), 'roofline': round(nbytes / ms / 1e9 / HBM_TBS, 3)}
    # lagged: forecast[f, t] against series[f + t], t < T - f; the forecast rows read once each, the series once
    sv = series[:T]
    row_bytes = 6 * N * N * C * 4
    lag_bytes = (sum(T - k for k in range(F)) + T) * row_bytes
    fl = Forecast(f, dims, co)
    sl = Forecast(sv, dims[1:], {d: co[d] for d in dims[1:]})
    sl.lat = vv.lat
    lag = {
        'lagged_rmse': lambda: forecast_error(f, sv, 'rmse'),
        'lagged_rmse_per_var': lambda: forecast_error(f, sv, 'rmse', axis=(0, 1, 2, 3)),
        'lagged_rmse_weighted_per_var': lambda: forecast_error(fl, sl, 'rmse', axis=(0, 1, 2, 3), weighted=True),
    }
    for k, fn in lag.items():
        ms = _time(fn, a.reps)
        out[k] = {'ms': round(ms, 3), 'TBs': round(lag_bytes / ms / 1e9, 3),
                  'roofline': round(lag_bytes / ms / 1e9 / HBM_TBS, 3)}
    if not a.no_host:
        fh, vh = f.cpu().numpy(), v.cpu().numpy()
        t0 = time.perf_counter()
        forecast_error(fh, vh, 'rmse')
        ms = 1e3 * (time.perf_counter() - t0)
        out['host_numpy_aligned_rmse'] = {'ms': round(ms, 1), 'TBs': round(nbytes / ms / 1e9, 4)}
        del fh, vh
    del f, v, series, fv, vv, fl, sl
    torch.cuda.empty_cache()
    if not a.no_end_to_end:
        out['end_to_end'] = _end_to_end(a.reps)
    print(json.dumps(out))


def _end_to_end(reps):
    """a C24 two-step model of the DLWP-CS configuration, 60 initialisations x 20 leads"""
    from DLWP.keras import backend
    backend.set_device('cuda:0')
    from DLWP.model import DLWPFunctional, TimeSeriesEstimator
    from DLWP.model.cs_unet import build_cs_model
    from DLWP.model.generators import ArrayDataGenerator
    from DLWP.verify import forecast_error
    N, V, K, T, ITS = 24, 4, 2, 120, 2
    rng = np.random.default_rng(1)
    arr = rng.standard_normal((T, V, 6, N, N)).astype(np.float32)
    sol = rng.random((T, 6, N, N)).astype(np.float32)
    const = rng.standard_normal((K, 6, N, N)).astype(np.float32)
    lat = rng.uniform(-89, 89, (6, N, N))
    dlwp = DLWPFunctional(is_convolutional=True, time_dim=ITS)
    gen = ArrayDataGenerator(dlwp, arr, rank=3, batch_size=8, input_time_steps=ITS, output_time_steps=ITS, sequence=2,
                             insolation_array=sol, constants=const, channels_last=True, device=True)
    np.random.seed(0)
    model = build_cs_model(gen.convolution_shape, ITS * V, 'unet2', base_filter_number=16, integration_steps=2, io_time_steps=ITS,
                           insolation_shape=gen.insolation_shape, constants_shape=(6, N, N, K))
    dlwp.build_model(model, loss='mse', optimizer='adam')
    est = TimeSeriesEstimator(dlwp, gen, lat=lat)
    samples = np.arange(60)
    steps = 20

    def device():
        return forecast_error(est.predict(steps, samples, keep_on_device=True), est.verification(steps, samples, keep_on_device=True),
                              'rmse', axis=(1, 2, 3, 4), weighted=True)

    def host():
        return forecast_error(est.predict(steps, samples), est.verification(steps, samples), 'rmse', axis=(1, 2, 3, 4),
                              weighted=True)
    d_ms, h_ms = _time(device, reps), _time(host, reps)
    err = float(np.nanmax(np.abs(device() - host()) / np.abs(host())))
    return {'device_ms': round(d_ms, 2), 'host_ms': round(h_ms, 2), 'max_rel_diff': err, 'leads': steps, 'inits': len(samples)}


if __name__ == '__main__':
    main()
