#!/usr/bin/env python3
"""
Spectra along time on the device: what they cost.  One JSON line.

`ops.time_spectrum` (dlwpcs_time_spectrum) on a 6-hourly C48 series of 4 variables (time, variable, face, height, width), fp32,
about --gb GB long: Welch's spectrum with segments of 512 rows, hop 256, a Hann window and the segment means removed, at 33
frequencies and at all 257.  Per case: milliseconds (device events, median of --reps calls after one warm-up call), the plan,
fp32 operations per second counted as 4 M per (segment, column, frequency), and the two lower bounds: one read of the series and
one write of the result at the device-to-device copy rate measured in the same run, and the operations at the 155 TFLOP/s of
v_mfma_f32_32x32x2_f32.  Beside it the torch route on the same tensor (unfold, subtract the mean, window, torch.fft.rfft,
abs() ** 2, mean over the segments) with the largest difference between the two results relative to the largest value.  Then
`verify.wavenumber_frequency_spectrum` on a (time, 48 latitudes, 144 longitudes) series of the same size: the whole call, and its
two stages alone.  The series have no NaN: the torch route has no notion of them.
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


def _torch_route(x, M, hop, w, K):
    seg = x.unfold(0, M, hop)                                   # (segments, ..., M), a view
    seg = (seg - seg.mean(dim=-1, keepdim=True)) * w
    p = torch.fft.rfft(seg, dim=-1)[..., :K].abs() ** 2
    c = torch.full((K,), 2.0, device=x.device)
    c[0] = 1.0
    if K == M // 2 + 1 and M % 2 == 0:
        c[-1] = 1.0
    return (p.mean(dim=0) * (c / (M * float((w ** 2).sum())))).movedim(-1, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--gb', type=float, default=1.0, help='size of the series')
    ap.add_argument('--segment', type=int, default=512)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_time_spectrum: no HIP device (times are measured on the GPU or not at all)')
    from DLWP import ops
    from DLWP import verify as V
    dev = torch.device('cuda:0')
    M, hop = a.segment, a.segment // 2
    per_row = 4 * 6 * 48 * 48
    T = max(2 * M, int(round(a.gb * 1e9 / (4.0 * per_row))))
    gen = torch.Generator(device=dev).manual_seed(1)
    src = 280.0 + 5.0 * torch.randn((T, 4, 6, 48, 48), dtype=torch.float32, device=dev, generator=gen)
    nbytes = 4.0 * src.numel()
    twin = torch.empty_like(src)
    copy_ms = _time(lambda: twin.copy_(src), a.reps)
    del twin
    copy_gbs = 2 * nbytes / copy_ms / 1e6
    n_seg = (T - M) // hop + 1
    out = {'reps': a.reps, 'device': torch.cuda.get_device_name(0), 'steps': T, 'series_GB': round(nbytes / 1e9, 3),
           'copy_GBs': round(copy_gbs, 1), 'segment': M, 'hop': hop, 'segments': n_seg}
    w = V.spectral_window('hann', M)
    wd = torch.as_tensor(w, dtype=torch.float32, device=dev)
    for K in (33, M // 2 + 1):
        flops = 4.0 * M * K * n_seg * per_row
        moved = nbytes + 4.0 * K * per_row
        ms = _time(lambda: ops.time_spectrum(src, None, M, hop, w, detrend=True, n_freq=K), a.reps)
        rec = {'plan': ops.time_spectrum_plan(src.shape, src.stride(), M, hop, n_freq=K), 'ms': round(ms, 3),
               'TFLOPs': round(flops / ms / 1e9, 2), 'bound_bytes_ms': round(moved / copy_gbs / 1e6, 3),
               'bound_flops_ms': round(flops / MFMA_F32_FLOPS * 1e3, 3)}
        ours = ops.time_spectrum(src, None, M, hop, w, detrend=True, n_freq=K)
        t_ms = _time(lambda: _torch_route(src, M, hop, wd, K), a.reps)
        ref = _torch_route(src, M, hop, wd, K)
        rec['torch_rfft'] = {'ms': round(t_ms, 3), 'over_ours': round(t_ms / ms, 2),
                             'max_rel_diff': float((ours - ref).abs().max() / ref.abs().max())}
        del ours, ref
        torch.cuda.empty_cache()
        out['n_freq_%d' % K] = rec
    del src
    torch.cuda.empty_cache()
    # the wavenumber-frequency diagram of a latitude-longitude series of the same size
    nlat, L = 48, 144
    T2 = max(2 * M, int(round(a.gb * 1e9 / (4.0 * nlat * L))))
    ll = torch.randn((T2, nlat, L), dtype=torch.float32, device=dev, generator=gen)
    wk = {'steps': T2, 'nlat': nlat, 'nlon': L, 'n_wave': 16, 'n_freq': 65}
    wk['ms'] = round(_time(lambda: V.wavenumber_frequency_spectrum(ll, M, n_wave=16, n_freq=65), a.reps), 3)
    wk['zonal_stage_ms'] = round(_time(lambda: ops.time_fourier(ll, row_axis=2, n_freq=16), a.reps), 3)
    z = ops.time_fourier(ll, row_axis=2, n_freq=16)[0]
    wk['time_stage_ms'] = round(_time(lambda: ops.time_spectrum(z[..., 0], z[..., 1], M, hop, w, detrend=True, n_freq=65), a.reps), 3)
    # the remedy named for a slow zonal stage: a copy with the columns along the lanes, its time included
    wk['zonal_stage_transposed_copy_ms'] = round(_time(lambda: ops.time_fourier(ll.permute(2, 0, 1).contiguous(), row_axis=0, n_freq=16),
                                                       a.reps), 3)
    out['wavenumber_frequency'] = wk
    print(json.dumps(out))


if __name__ == '__main__':
    main()
