#!/usr/bin/env python3
"""
The row Gram matrix on the device: what it costs.  One JSON line.

`ops.row_gram` (dlwpcs_row_gram) on an fp32 series of 1 GiB at (rows, columns) = (128, 2097152), (512, 524288) and
(2048, 131072) (--scale multiplies the columns), centred on its own mean and weighted, in the symmetric form and in the cross form against 15 rows (projection
onto patterns).  Per case: milliseconds (device events, median of --reps calls after one warm-up call), the plan, the fraction
of the two-pass floor (the column pass and the products read the series once each: two reads at the device-to-device copy rate
measured in the same run), and fp32-matrix TFLOP/s counted as 2 Ta Tb E (the symmetric form computes the tile pairs on or below
the diagonal only, so its useful rate is quoted against the full product as a BLAS would be).  Beside it the torch expression
y = (x - x.mean(0)) * r; y @ y.T in fp32 and with .double(), the bytes of the temporary it allocates, and the largest
difference between the results relative to the largest value.  The series have no NaN: the torch route has no notion of them.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'dlwp-cs_amd')]

import numpy as np   # noqa: E402
import torch         # noqa: E402

MFMA_F32_FLOPS = 155e12
SHAPES = ((128, 2097152), (512, 524288), (2048, 131072))


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


def _torch_route(x, r, double):
    y = (x - x.mean(0)) * r
    if double:
        y = y.double()
    return y @ y.T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--scale', type=float, default=1.0, help='multiplies the column counts (1: series of 1 GiB)')
    ap.add_argument('--no-double', action='store_true', help='skip the fp64 torch route')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_row_gram: no HIP device (times are measured on the GPU or not at all)')
    from DLWP import ops
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(1)
    out = {'reps': a.reps, 'device': torch.cuda.get_device_name(0)}
    for T, E0 in SHAPES:
        E = max(512, int(round(E0 * a.scale)) // 512 * 512)
        x = 280.0 + 10.0 * torch.randn((T, E), dtype=torch.float32, device=dev, generator=gen)
        r = torch.sqrt((0.2 + 0.8 * torch.rand((E,), dtype=torch.float32, device=dev, generator=gen)) / E)
        pat = torch.randn((15, E), dtype=torch.float32, device=dev, generator=gen)
        nbytes = 4.0 * x.numel()
        twin = torch.empty_like(x)
        copy_ms = _time(lambda: twin.copy_(x), a.reps)
        del twin
        copy_gbs = 2 * nbytes / copy_ms / 1e6
        floor_ms = 2 * nbytes / copy_gbs / 1e6
        rec = {'series_GB': round(nbytes / 1e9, 3), 'copy_GBs': round(copy_gbs, 1), 'two_pass_floor_ms': round(floor_ms, 3)}
        flops = 2.0 * T * T * E
        for name, split in (('chosen', None), ('walk', False)):
            ms = _time(lambda: ops.row_gram(x, weight_root=r, split=split), a.reps)
            rec['symmetric_' + name] = {'plan': ops.row_gram_plan(x.shape, x.stride(), split=split), 'ms': round(ms, 3),
                                        'floor_fraction': round(floor_ms / ms, 3), 'TFLOPs': round(flops / ms / 1e9, 2),
                                        'bound_flops_ms': round(flops / 2 / MFMA_F32_FLOPS * 1e3, 3)}
        ms = _time(lambda: ops.row_gram(x, pat, weight_root=r, center_b=False), a.reps)
        rec['cross_15'] = {'plan': ops.row_gram_plan(x.shape, x.stride(), n_rows_b=15), 'ms': round(ms, 3),
                           'floor_fraction': round(floor_ms / ms, 3),
                           'TFLOPs': round(2.0 * T * 15 * E / ms / 1e9, 2)}
        ours = ops.row_gram(x, weight_root=r)
        t_ms = _time(lambda: _torch_route(x, r, False), a.reps)
        ref = _torch_route(x, r, False)
        rec['torch_fp32'] = {'ms': round(t_ms, 3), 'TFLOPs': round(flops / t_ms / 1e9, 2), 'temporary_bytes': int(nbytes),
                             'max_rel_diff': float((ours - ref.double()).abs().max() / ours.abs().max())}
        del ref
        if not a.no_double:
            t_ms = _time(lambda: _torch_route(x, r, True), a.reps)
            ref = _torch_route(x, r, True)
            rec['torch_fp64'] = {'ms': round(t_ms, 3), 'temporary_bytes': int(3 * nbytes),
                                 'max_rel_diff': float((ours - ref).abs().max() / ours.abs().max())}
            del ref
        del ours, x, r, pat
        torch.cuda.empty_cache()
        out['%dx%d' % (T, E)] = rec
    print(json.dumps(out))


if __name__ == '__main__':
    main()
