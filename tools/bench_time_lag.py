#!/usr/bin/env python3
"""
Lagged covariances along time on the device: what they cost.  One JSON line.

`ops.time_lag` (dlwpcs_time_lag) on a 6-hourly C48 series of 4 variables (time, variable, face, height, width), fp32, about --gb
GB long, with the centres of one `ops.group_mean` pass (timed apart): the autocovariance at the lags 0 .. 8 and 0 .. 32, the pair
form at -16 .. 16 and the index form at -20 .. 20, each on a complete series and with 1 % NaN.  Per case: milliseconds (device
events, median of --reps calls after one warm-up call), the plan, the bytes a pass reads (the series once, in the pair form
twice) and the lower bound passes x those bytes at the device-to-device copy rate measured in the same run.  Beside it the torch
route on the same tensors: per lag two shifted slices, a product, nan_to_num, a float64 sum and the count of the pairs present,
with the largest difference between the two results relative to the largest value.  --plans also times every forced lag block
under both split forms, and the one-element chunks of a view offset by one element.  Then what `verify.lag_correlation` pays in
its pair form on top of `verify.lag_covariance`: the two one-lag variance calls and their two mean passes.
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


def _torch_route(a, b, lags, ca, cb):
    """per lag: shifted slices, a product, nan_to_num, a float64 sum over the count of the pairs present"""
    T = a.shape[0]
    da = a - ca
    db = da if b is None else (b - cb if b.dim() > 1 else (b - cb).reshape((T,) + (1,) * (a.dim() - 1)))
    out = []
    for l in lags:
        t0, t1 = max(0, -l), min(T, T - l)
        p = da[t0:t1] * db[t0 + l:t1 + l]
        n = (~torch.isnan(p)).sum(dim=0)
        out.append((torch.nan_to_num(p).sum(dim=0, dtype=torch.float64) / n).to(torch.float32))
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--gb', type=float, default=1.0, help='size of the series')
    ap.add_argument('--plans', action='store_true', help='also time every forced lag block, both split forms and the scalar chunks')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_time_lag: no HIP device (times are measured on the GPU or not at all)')
    from DLWP import ops
    from DLWP import verify as V
    dev = torch.device('cuda:0')
    per_row = 4 * 6 * 48 * 48
    T = max(64, int(round(a.gb * 1e9 / (4.0 * per_row))))
    gen = torch.Generator(device=dev).manual_seed(1)
    shape = (T, 4, 6, 48, 48)
    x = 280.0 + 5.0 * torch.randn(shape, dtype=torch.float32, device=dev, generator=gen)
    y = 10.0 + 2.0 * torch.randn(shape, dtype=torch.float32, device=dev, generator=gen)
    idx = torch.randn((T,), dtype=torch.float32, device=dev, generator=gen)
    nbytes = 4.0 * x.numel()
    twin = torch.empty_like(x)
    copy_ms = _time(lambda: twin.copy_(x), a.reps)
    del twin
    copy_gbs = 2 * nbytes / copy_ms / 1e6
    out = {'reps': a.reps, 'device': torch.cuda.get_device_name(0), 'steps': T, 'columns': per_row, 'series_GB': round(nbytes / 1e9, 3),
           'copy_GBs': round(copy_gbs, 1)}
    mean = lambda t: ops.group_mean(t, [0, T], np.arange(T), row_axis=0)     # noqa: E731
    out['mean_pass_ms'] = round(_time(lambda: mean(x), a.reps), 3)
    cases = (('auto_0_8', 'auto', list(range(0, 9))), ('auto_0_32', 'auto', list(range(0, 33))),
             ('pair_-16_16', 'pair', list(range(-16, 17))), ('index_-20_20', 'index', list(range(-20, 21))))
    for missing in (False, True):
        if missing:
            x = torch.where(torch.rand(shape, device=dev, generator=gen) < 0.01, torch.full_like(x, float('nan')), x)
            y = torch.where(torch.rand(shape, device=dev, generator=gen) < 0.01, torch.full_like(y, float('nan')), y)
        cx, cy, ci = mean(x), mean(y), mean(idx)
        for name, form, lags in cases:
            b, cb = {'auto': (None, None), 'pair': (y, cy), 'index': (idx, ci)}[form]
            run = lambda **kw: ops.time_lag(x, b, lags=lags, center_a=cx, center_b=cb, **kw)     # noqa: E731
            plan = ops.time_lag_plan(x.shape, x.stride(), len(lags), form=form)
            ms = _time(run, a.reps)
            pass_bytes = nbytes * (2 if form == 'pair' else 1)
            rec = {'plan': plan, 'ms': round(ms, 3), 'pass_MB': round(pass_bytes / 1e6, 1),
                   'bound_ms': round(plan['passes'] * pass_bytes / copy_gbs / 1e6, 3)}
            ours = run()
            route = lambda: _torch_route(x, b, lags, cx, cb)       # noqa: E731
            t_ms = _time(route, a.reps)
            ref = route()
            diff = ((ours - ref).abs() / ref.nan_to_num(0.0).abs().max()).nan_to_num(0.0, 0.0, 0.0)
            rec['torch'] = {'ms': round(t_ms, 3), 'over_ours': round(t_ms / ms, 2), 'max_rel_diff': float(diff.max())}
            del ours, ref, diff
            if a.plans:
                forced = {}
                for split in (False, True):
                    for block in (1, 4, 8, 16):
                        p = ops.time_lag_plan(x.shape, x.stride(), len(lags), form=form, split=split, lag_block=block)
                        forced['split%d_block%d' % (split, block)] = {
                            'ms': round(_time(lambda: run(split=split, lag_block=block), a.reps), 3), 'passes': p['passes'],
                            'scratch_MB': round(p['scratch_bytes'] / 1e6, 1)}
                rec['forced'] = forced
            torch.cuda.empty_cache()
            out[name + ('_nan' if missing else '')] = rec
        if a.plans and not missing:
            # the one-element chunks: the same series one element off a 16-byte boundary
            buf = torch.empty(x.numel() + 4, dtype=torch.float32, device=dev)
            xs = buf[1:1 + x.numel()].view(shape)
            xs.copy_(x)
            lags = list(range(0, 33))
            scalar = {}
            for split in (None, False, True):
                for block in (None, 8, 16):
                    p = ops.time_lag_plan(shape, xs.stride(), len(lags), split=split, lag_block=block, aligned=False)
                    scalar['split%s_block%s' % (split, block)] = {
                        'ms': round(_time(lambda: ops.time_lag(xs, lags=lags, center_a=cx, split=split, lag_block=block), a.reps), 3),
                        'vec': p['vec'], 'passes': p['passes'], 'split': p['split']}
            out['auto_0_32_scalar_chunks'] = scalar
            # a longer step: the partners are loaded row by row
            lags4 = list(range(-32, 33, 4))
            out['auto_step4_17_lags'] = {'ms': round(_time(lambda: ops.time_lag(x, lags=lags4, center_a=cx), a.reps), 3),
                                         'plan': ops.time_lag_plan(x.shape, x.stride(), len(lags4), lag_step=4)}
            del buf, xs
            torch.cuda.empty_cache()
    # what the pair form of lag_correlation pays on top of the covariance (on the series with NaN)
    lags = list(range(-16, 17))
    cov = _time(lambda: V.lag_covariance(x, y, lags), a.reps)
    cor = _time(lambda: V.lag_correlation(x, y, lags), a.reps)
    one = _time(lambda: ops.time_lag(x, lags=[0], center_a=cx), a.reps)
    out['lag_correlation_pair'] = {'covariance_ms': round(cov, 3), 'correlation_ms': round(cor, 3), 'extra_ms': round(cor - cov, 3),
                                   'one_lag_auto_ms': round(one, 3), 'mean_pass_ms': out['mean_pass_ms']}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
