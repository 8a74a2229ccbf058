#!/usr/bin/env python3
"""
Least-squares fits along time on the device: what they cost.  One JSON line.

`ops.time_regression` (dlwpcs_time_regression) on the series of bench_time_filter.py: 6-hourly C48 data of 4 variables (time,
variable, face, height, width), fp32, about --gb GB long.  K = 2 (mean and trend), 10 (mean, trend, 4 harmonics) and 16 terms, on
complete data and with 1 % NaN (every column then has gaps and needs a normal matrix of its own), in both gram forms; and
`ops.time_regression_apply` in residual mode.  Per case: milliseconds (device events, median of --reps calls after one warm-up
call), GB/s over one read of the series (apply: a read and a write), that rate over the device-to-device copy rate measured in the
same run (`of_copy`), fp64 fused multiply-adds per second (K per element and row for the streaming sums, K (K + 1) / 2 more for a
column's own normal matrix) and the plan.  Beside it the torch route on the same tensor: complete data, basis^T @ x and one
torch.linalg.solve; data with gaps, the masked products (b_i b_j)^T @ mask and a batched solve per column, with the largest
difference between the coefficients relative to the largest coefficient.
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


def _torch_complete(x, b):
    """basis^T @ x in fp32 (what torch does at speed), the K x K system in fp64"""
    T = x.shape[0]
    c = (b.t() @ x.reshape(T, -1)).double()
    G = (b.t() @ b).double()
    return torch.linalg.solve(G, c).float().reshape((b.shape[1],) + tuple(x.shape[1:]))


def _torch_gappy(x, b):
    T, K = b.shape
    v = x.reshape(T, -1)
    mask = ~torch.isnan(v)
    c = (b.t() @ torch.where(mask, v, torch.zeros_like(v))).double()                        # (K, E)
    bb = (b[:, :, None] * b[:, None, :]).reshape(T, K * K)
    G = (bb.t() @ mask.float()).double().reshape(K, K, -1).permute(2, 0, 1)              # (E, K, K)
    a = torch.linalg.solve(G, c.t()[:, :, None])[:, :, 0]
    return a.t().float().reshape((K,) + tuple(x.shape[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--gb', type=float, default=1.0, help='size of the series')
    ap.add_argument('--no-torch', action='store_true', help='skip the torch routes')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_time_regression: no HIP device (times are measured on the GPU or not at all)')
    from DLWP import ops
    dev = torch.device('cuda:0')
    per_row = 4 * 6 * 48 * 48
    T = max(256, int(round(a.gb * 1e9 / (4.0 * per_row))))
    gen = torch.Generator(device=dev).manual_seed(1)
    src = 280.0 + 5.0 * torch.randn((T, 4, 6, 48, 48), dtype=torch.float32, device=dev, generator=gen)
    gappy = src.clone()
    gappy[torch.rand(src.shape, device=dev, generator=gen) < 0.01] = float('nan')
    nbytes = 4.0 * src.numel()
    twin = torch.empty_like(src)
    copy_ms = _time(lambda: twin.copy_(src), a.reps)
    copy_gbs = 2 * nbytes / copy_ms / 1e6
    out = {'reps': a.reps, 'device': torch.cuda.get_device_name(0), 'rows': T, 'series_GB': round(nbytes / 1e9, 3),
           'copy_GBs': round(copy_gbs, 1)}
    t = np.arange(T, dtype=np.float64)
    year = 4 * 365.24219

    def basis(K):
        cols = [np.ones(T), (2. * t - (T - 1)) / (T - 1)]
        h = 1
        while len(cols) < K:
            cols += [np.cos(2. * np.pi * h * t / year), np.sin(2. * np.pi * h * t / year)]
            h += 1
        return torch.as_tensor(np.stack(cols[:K], axis=1), dtype=torch.float32, device=dev).contiguous()

    for K in (2, 10, 16):
        b = basis(K)
        for name, x in (('complete', src), ('nan1pct', gappy)):
            rec = {'terms': K, 'plan': ops.time_regression_plan(x.shape, x.stride(), K)}
            for gram in (False, True):
                ms = _time(lambda: ops.time_regression(x, b, gram=gram), a.reps)
                own = gram or name != 'complete'
                fma = (K + (K * (K + 1) // 2 if own else 0)) * float(src.numel())
                gbs = nbytes / ms / 1e6
                rec['own_gram' if gram else 'shared_factor'] = {'ms': round(ms, 3), 'GBs': round(gbs, 1), 'of_copy': round(gbs / copy_gbs, 3),
                                                                'Gfma_s': round(fma / ms / 1e6, 1)}
            if not a.no_torch:
                ours = ops.time_regression(x, b)
                fn = (lambda: _torch_complete(x, b)) if name == 'complete' else (lambda: _torch_gappy(x, b))
                t_ms = _time(fn, a.reps)
                theirs = fn()
                rec['torch'] = {'ms': round(t_ms, 3), 'over_ours': round(t_ms / rec['shared_factor']['ms'], 2),
                                'max_rel_diff': float(((ours - theirs).abs().amax(dim=0) / ours.abs().amax(dim=0)).max())}
                del ours, theirs
                torch.cuda.empty_cache()
            out['K%d_%s' % (K, name)] = rec
    b = basis(10)
    coef = ops.time_regression(src, b)
    ms = _time(lambda: ops.time_regression_apply(coef, b, src=src), a.reps)
    gbs = 2 * nbytes / ms / 1e6
    out['apply_residual_K10'] = {'ms': round(ms, 3), 'GBs': round(gbs, 1), 'of_copy': round(gbs / copy_gbs, 3),
                                 'Gfma_s': round(10 * float(src.numel()) / ms / 1e6, 1)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
