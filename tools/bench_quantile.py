#!/usr/bin/env python3
"""
Climatological quantiles on the device: what they cost.  One JSON line.

`ops.group_quantile` (dlwpcs_group_quantile): the terciles of a 6-hourly C48 series of 4 variables (time, variable, face, height,
width), fp32, about --gb GB long, grouped by day of the year, by month and as one group.  Per grouping: milliseconds (device
events, median of --reps calls after one warm-up call), GB/s over the bytes of ONE read of the series, that rate over the
device-to-device copy rate of the series in the same run (`of_copy`), the plan (form, class, grid), and the same numbers from a
torch composition on the same tensors as the yardstick: per group an index_select of its rows, `torch.sort` along time, two gathers
and a lerp (its time, and the largest difference between the two results).  The series has no NaN (the yardstick has no notion of
them); the groups are the calendar's.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'dlwp-cs_amd')]

import numpy as np   # noqa: E402
import torch         # noqa: E402

PROBS = (1.0 / 3.0, 2.0 / 3.0)


def _time(fn, reps):
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


def _torch_route(src, groups):
    out = torch.empty((len(PROBS), len(groups)) + tuple(src.shape[1:]), dtype=torch.float32, device=src.device)
    for k, idx in enumerate(groups):
        xs = torch.sort(src.index_select(0, idx), dim=0).values
        n = xs.shape[0]
        for q, p in enumerate(PROBS):
            h = (n - 1) * p
            j = int(np.floor(h))
            out[q, k] = torch.lerp(xs[j], xs[min(j + 1, n - 1)], float(h - j))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--gb', type=float, default=1.0, help='size of the series')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_quantile: no HIP device (times are measured on the GPU or not at all)')
    from DLWP import ops
    from DLWP import verify as V
    dev = torch.device('cuda:0')
    per_row = 4 * 6 * 48 * 48
    T = max(8, int(round(a.gb * 1e9 / (4.0 * per_row))))
    times = np.datetime64('1979-01-01T00') + 6 * np.arange(T).astype('timedelta64[h]')
    gen = torch.Generator(device=dev).manual_seed(1)
    src = 280.0 + 5.0 * torch.randn((T, 4, 6, 48, 48), dtype=torch.float32, device=dev, generator=gen)
    nbytes = 4.0 * src.numel()
    twin = torch.empty_like(src)
    copy_ms = _time(lambda: twin.copy_(src), a.reps)
    del twin
    copy_gbs = 2 * nbytes / copy_ms / 1e6
    out = {'reps': a.reps, 'device': torch.cuda.get_device_name(0), 'steps': T, 'series_GB': round(nbytes / 1e9, 3),
           'copy_GBs': round(copy_gbs, 1), 'probs': list(PROBS)}
    for by in ('dayofyear', 'month', None):
        keys = np.zeros(T, dtype=np.int64) if by is None else V.calendar_keys(times, by)
        _, start, order = V._csr(keys)
        groups = [torch.from_numpy(order[start[k]:start[k + 1]]).to(dev) for k in range(len(start) - 1)]
        plan = ops.group_quantile_plan(src.shape, src.stride(), len(groups), int(np.diff(start).max()), len(PROBS))
        ms = _time(lambda: ops.group_quantile(src, start, order, PROBS), a.reps)
        t_ms = _time(lambda: _torch_route(src, groups), a.reps)
        ours, theirs = ops.group_quantile(src, start, order, PROBS), _torch_route(src, groups)
        gbs = nbytes / ms / 1e6
        out[str(by)] = {'groups': len(groups), 'longest': int(np.diff(start).max()), 'plan': plan, 'ms': round(ms, 3),
                        'GBs': round(gbs, 1), 'of_copy': round(gbs / copy_gbs, 3), 'torch_ms': round(t_ms, 3),
                        'torch_over_ours': round(t_ms / ms, 2), 'max_abs_diff': float((ours - theirs).abs().max())}
        del ours, theirs, groups
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
