#!/usr/bin/env python3
"""
Per-variable scaling on the device (DLWP.model.preprocessing -> dlwpcs_channel_moments / dlwpcs_channel_affine) against the same
results computed with plain torch expressions in the same process, and against the device-to-device copy rate: one JSON line.

  * resident: a (T, 4, 6, 48, 48) fp32 array of about --gb GB (the training array, channels-first).
      moments    one `ops.channel_moments` call (all four variables, both sums)   vs  x.double().sum(...) and
                 ((x.double() - m) ** 2).sum(...) -- the two passes `variable_statistics` replaces, each timed
      transform  `VariableScaler.transform(x, out=x)`, in place                   vs  (x - m) / s, broadcast, into a new array
  * forecast: a (40, 32, 6, 48, 48, 4) fp32 forecast (channels-last, what predict() returns).
      inverse_in_place       `inverse_transform(f, out=f)`                        vs  f * s + m, broadcast
      inverse_channels_first `inverse_transform(f, channels_first=True)`          vs  (f * s + m).permute(0, 1, 5, 2, 3, 4).contiguous()
      moments_channels_last  `ops.channel_moments(f, axis=-1)`, the one-element path  vs  the two torch passes over axis -1
  * copy: `dst.copy_(src)` of the same arrays, the device-to-device rate of the same run.
Device events around each call, median of --reps calls after one warm-up call.  GB/s counts the bytes a step has to move: the
array once for the moments, read + write for the transforms and the copy; `of_copy` is that rate over the copy's.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'dlwp-cs_amd')]

import numpy as np   # noqa: E402
import torch         # noqa: E402


def _time(fn, reps):
    """median milliseconds of fn() over `reps` calls after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def _entry(ms, nbytes, copy_gbs, torch_ms=None):
    gbs = nbytes / ms / 1e6
    out = {'ms': round(ms, 3), 'GBs': round(gbs, 1), 'of_copy': round(gbs / copy_gbs, 3)}
    if torch_ms is not None:
        out['torch_ms'] = round(torch_ms, 3)
        out['torch_over_ours'] = round(torch_ms / ms, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gb', type=float, default=2.0, help='size of the resident array')
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_scaling: no HIP device (times are measured on the GPU or not at all)')
    from DLWP import ops
    from DLWP.model.preprocessing import VariableScaler
    dev = torch.device('cuda:0')
    V, S = 4, 6 * 48 * 48
    T = int(a.gb * 1e9 / (V * S * 4))
    mean = np.array([0.1, -0.2, 0.05, 0.3], dtype=np.float32)
    std = np.array([1.05, 0.95, 1.1, 0.9], dtype=np.float32)
    sc = VariableScaler(mean, std)
    out = {'resident_shape': [T, V, 6, 48, 48], 'forecast_shape': [40, 32, 6, 48, 48, V], 'reps': a.reps,
           'device': torch.cuda.get_device_name(0)}

    # ---- the resident array ----
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((T, V, 6, 48, 48), dtype=torch.float32, device=dev, generator=gen)
    y = torch.empty_like(x)
    nbytes = x.numel() * 4
    copy_ms = _time(lambda: y.copy_(x), a.reps)
    copy_gbs = 2 * nbytes / copy_ms / 1e6
    res = {'MB': round(nbytes / 1e6, 1), 'copy': {'ms': round(copy_ms, 3), 'GBs': round(copy_gbs, 1)}}
    del y
    m_dev = torch.from_numpy(mean.astype(np.float64)).to(dev)
    t_sum = _time(lambda: x.double().sum((0, 2, 3, 4)), a.reps)
    t_sq = _time(lambda: ((x.double() - m_dev.reshape(1, V, 1, 1, 1)) ** 2).sum((0, 2, 3, 4)), a.reps)
    ours = _time(lambda: ops.channel_moments(x, axis=1, center=m_dev), a.reps)
    res['moments'] = _entry(ours, nbytes, copy_gbs, t_sum + t_sq)
    res['moments']['torch_sum_ms'], res['moments']['torch_squares_ms'] = round(t_sum, 3), round(t_sq, 3)
    mt, st = sc._tables(dev)
    t_tr = _time(lambda: (x - mt.reshape(1, V, 1, 1, 1)) / st.reshape(1, V, 1, 1, 1), a.reps)
    ours = _time(lambda: sc.transform(x, out=x), a.reps)
    res['transform_in_place'] = _entry(ours, 2 * nbytes, copy_gbs, t_tr)
    out['resident'] = res
    del x
    torch.cuda.empty_cache()

    # ---- the forecast ----
    f = torch.randn((40, 32, 6, 48, 48, V), dtype=torch.float32, device=dev, generator=gen)
    g = torch.empty_like(f)
    nbytes = f.numel() * 4
    copy_ms = _time(lambda: g.copy_(f), a.reps)
    copy_gbs = 2 * nbytes / copy_ms / 1e6
    fc = {'MB': round(nbytes / 1e6, 1), 'copy': {'ms': round(copy_ms, 3), 'GBs': round(copy_gbs, 1)}}
    t_inv = _time(lambda: f * st + mt, a.reps)
    t_cf = _time(lambda: (f * st + mt).permute(0, 1, 5, 2, 3, 4).contiguous(), a.reps)
    t_perm = _time(lambda: f.permute(0, 1, 5, 2, 3, 4).contiguous(), a.reps)
    cf = g.view(40, 32, V, 6, 48, 48)
    ours_cf = _time(lambda: sc.inverse_transform(f, axis=-1, out=cf, channels_first=True), a.reps)
    ours = _time(lambda: sc.inverse_transform(f, axis=-1, out=f), a.reps)
    fc['inverse_in_place'] = _entry(ours, 2 * nbytes, copy_gbs, t_inv)
    fc['inverse_channels_first'] = _entry(ours_cf, 2 * nbytes, copy_gbs, t_cf)
    fc['inverse_channels_first']['torch_permute_only_ms'] = round(t_perm, 3)
    t_sum = _time(lambda: f.double().sum((0, 1, 2, 3, 4)), a.reps)
    t_sq = _time(lambda: ((f.double() - m_dev) ** 2).sum((0, 1, 2, 3, 4)), a.reps)
    ours = _time(lambda: ops.channel_moments(f, axis=-1, center=m_dev), a.reps)
    fc['moments_channels_last'] = _entry(ours, nbytes, copy_gbs, t_sum + t_sq)
    out['forecast'] = fc
    print(json.dumps(out))


if __name__ == '__main__':
    main()
