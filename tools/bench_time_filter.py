#!/usr/bin/env python3
"""
Filters along time on the device: what they cost.  One JSON line.

`ops.time_filter` (dlwpcs_time_filter) on a 6-hourly C48 series of 4 variables (time, variable, face, height, width), fp32, about
--gb GB long: the weekly running mean (28 taps of one, mode 'mean', every entry required) at steps 1, 4 and 28, a 16-row mean at step 1, and a
121-tap Lanczos band-pass (2 to 6 days, mode 'sum') at step 1.  Per case and per form that can run it: milliseconds (device events, median of
--reps calls after one warm-up call), GB/s over the bytes of one read of the series and one write of the result, that rate over
the device-to-device copy rate measured in the same run (`of_copy`), fp32 operations per second counted as 2 K per output
element, and the plan.  Beside it the torch route on the same tensor: cumsum differences for the boxcar, and for the Lanczos taps
K scaled slices added up (--conv1d: also conv1d on a permuted copy, the copy's time included), with the largest difference
between the two results.  The series has no NaN: the torch routes have no notion of them.
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


def _boxcar(x, K, s):
    c = torch.cumsum(x, dim=0)
    out = c[K - 1:].clone()
    out[1:] -= c[:-K]
    return (out / K)[::s]


def _slices(x, h, J):
    out = torch.zeros((J,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    for k, hk in enumerate(h):
        out.add_(x[k:k + J], alpha=float(hk))
    return out


def _conv1d(x, h, J):
    cols = x.reshape(x.shape[0], -1).t().contiguous()
    w = torch.as_tensor(h, dtype=torch.float32, device=x.device).reshape(1, 1, -1)
    return torch.nn.functional.conv1d(cols[:, None, :], w)[:, 0, :].t().reshape((J,) + tuple(x.shape[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--gb', type=float, default=1.0, help='size of the series')
    ap.add_argument('--conv1d', action='store_true', help='also time conv1d on a permuted copy for the Lanczos taps')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_time_filter: no HIP device (times are measured on the GPU or not at all)')
    from DLWP import ops
    from DLWP import verify as V
    dev = torch.device('cuda:0')
    per_row = 4 * 6 * 48 * 48
    T = max(256, int(round(a.gb * 1e9 / (4.0 * per_row))))
    gen = torch.Generator(device=dev).manual_seed(1)
    src = 280.0 + 5.0 * torch.randn((T, 4, 6, 48, 48), dtype=torch.float32, device=dev, generator=gen)
    nbytes = 4.0 * src.numel()
    twin = torch.empty_like(src)
    copy_ms = _time(lambda: twin.copy_(src), a.reps)
    del twin
    copy_gbs = 2 * nbytes / copy_ms / 1e6
    out = {'reps': a.reps, 'device': torch.cuda.get_device_name(0), 'steps': T, 'series_GB': round(nbytes / 1e9, 3),
           'copy_GBs': round(copy_gbs, 1)}
    band = V.lanczos_weights(60, 1. / 24., 1. / 8.)
    cases = [('weekly_mean_step%d' % s, np.ones(28), s, 'mean', 28.) for s in (1, 4, 28)] + \
        [('mean16_step1', np.ones(16), 1, 'mean', 16.), ('lanczos121_step1', band, 1, 'sum', 0.)]
    for name, h, s, mode, mw in cases:
        K = len(h)
        J = (T - K) // s + 1
        hd = torch.as_tensor(h, dtype=torch.float32, device=dev)
        moved = nbytes * min(1., K / s) + 4.0 * J * per_row
        rec = {'taps': K, 'step': s, 'outputs': J}
        for form in ('streaming', 'gather'):
            try:
                plan = ops.time_filter_plan(src.shape, src.stride(), K, step=s, mode=mode, form=form)
            except ValueError:
                continue                                    # (more live outputs than the streaming form holds)
            ms = _time(lambda: ops.time_filter(src, hd, step=s, mode=mode, min_weight=mw, form=form), a.reps)
            gbs = moved / ms / 1e6
            rec[form] = {'plan': plan, 'ms': round(ms, 3), 'GBs': round(gbs, 1), 'of_copy': round(gbs / copy_gbs, 3),
                         'Gop_s': round(2.0 * K * J * per_row / ms / 1e6, 1)}
        rec['chosen'] = ops.time_filter_plan(src.shape, src.stride(), K, step=s, mode=mode)['form']
        ours = ops.time_filter(src, hd, step=s, mode=mode, min_weight=mw)
        routes = {'cumsum': lambda: _boxcar(src, K, s)} if mode == 'mean' else {'slices': lambda: _slices(src, h, J)}
        if mode == 'sum' and a.conv1d:
            routes['conv1d'] = lambda: _conv1d(src, h, J)
        for rname, fn in routes.items():
            t_ms = _time(fn, a.reps)
            rec['torch_' + rname] = {'ms': round(t_ms, 3), 'over_ours': round(t_ms / rec[rec['chosen']]['ms'], 2),
                                     'max_abs_diff': float((ours - fn()).abs().max())}
            torch.cuda.empty_cache()
        out[name] = rec
        del ours
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
