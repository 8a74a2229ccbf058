#!/usr/bin/env python3
"""
Zonal spectra on the device: what they cost.  One JSON line.

`ops.zonal_spectrum` (dlwpcs_zonal_spectrum), single and pair form, over forecasts laid out (lead, time, variable, lat, lon):
(40, 32, 4, 181, 360) and (8, 8, 4, 721, 1440) fp32, averaged over time and a cosine-weighted latitude band per lead and
variable.  Per case and form: milliseconds (device events, median of --reps calls after one warm-up call), the fraction of the
fp32 matrix peak with 2 L 2K flops per row (twice that for the pair form), bytes read per second, the peak device memory of
the call, and the same result from `torch.fft.rfft` plus torch reductions on the same tensors as the yardstick (its time, its
peak memory, the largest difference between the two results relative to the largest value).  --n-wave adds the same calls
restricted to the first wavenumbers.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'dlwp-cs_amd')]

import numpy as np   # noqa: E402
import torch         # noqa: E402

PEAK_F32_MATRIX = 155e12          # flop/s, v_mfma_f32_32x32x2_f32 on all 256 compute units


def _time(fn, reps):
    """(median milliseconds of fn() over `reps` calls after one warm-up call, peak bytes allocated above the resting level)"""
    fn()
    torch.cuda.synchronize()
    rest = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), int(torch.cuda.max_memory_allocated() - rest)


def _torch_route(f, v, w, K):
    """the yardstick: rfft, powers, rows that count, weighted mean over (time, lat); (nq, lead, variable, K)"""
    L = f.shape[-1]
    ck = torch.full((K,), 2.0, device=f.device)
    ck[0] = 1.0
    if L % 2 == 0 and K == L // 2 + 1:
        ck[-1] = 1.0
    ck = ck / float(L * L)
    F = torch.fft.rfft(f, dim=-1)[..., :K]
    ok = torch.isfinite(f).all(dim=-1)
    q = [F.real ** 2 + F.imag ** 2]
    if v is not None:
        V = torch.fft.rfft(v, dim=-1)[..., :K]
        ok = ok & torch.isfinite(v).all(dim=-1)
        cross = F * torch.conj(V)
        q += [V.real ** 2 + V.imag ** 2, cross.real, cross.imag]
    ww = (w * ok)[..., None].double()                                   # (lead, time, variable, lat, 1)
    sw = ww.sum(dim=(1, 3))
    return torch.stack([(torch.where(ok[..., None], x, torch.zeros_like(x)) * ck * ww).sum(dim=(1, 3)) / sw for x in q])


def _case(shape, reps, n_wave, dev):
    from DLWP import ops
    gen = torch.Generator(device=dev).manual_seed(3)
    f = torch.randn(shape, dtype=torch.float32, device=dev, generator=gen)
    v = torch.roll(f, 2, dims=-1) + 0.5 * torch.randn(shape, dtype=torch.float32, device=dev, generator=gen)
    lat = torch.linspace(-90., 90., shape[3], device=dev)
    w = (torch.cos(torch.deg2rad(lat)) * (lat.abs() <= 60.)).float()    # a band: zeros and ones times cos(lat)
    L = shape[-1]
    rows = int(np.prod(shape[:-1]))
    out = {'shape': list(shape), 'rows': rows, 'groups': shape[0] * shape[2]}
    for K in [L // 2 + 1] + ([n_wave] if n_wave and n_wave < L // 2 + 1 else []):
        res = {}
        for form, b in (('single', None), ('pair', v)):
            nq = 1 if b is None else 2
            nw = None if K == L // 2 + 1 else K
            ms, peak = _time(lambda: ops.zonal_spectrum(f, b, reduced=(1, 3), weights=w, n_wave=nw), reps)
            t_ms, t_peak = _time(lambda: _torch_route(f, b, w, K), reps)
            ours = ops.zonal_spectrum(f, b, reduced=(1, 3), weights=w, n_wave=nw).double()
            theirs = _torch_route(f, b, w, K)
            ours = ours[None] if b is None else ours
            flops = 2.0 * L * 2 * K * rows * nq
            nbytes = 4.0 * L * rows * nq
            res[form] = {'ms': round(ms, 3), 'of_f32_matrix_peak': round(flops / (ms * 1e-3) / PEAK_F32_MATRIX, 4),
                         'GBs': round(nbytes / ms / 1e6, 1), 'peak_MB': round(peak / 1e6, 2), 'torch_ms': round(t_ms, 3),
                         'torch_peak_MB': round(t_peak / 1e6, 1), 'torch_over_ours': round(t_ms / ms, 2),
                         'max_rel_diff': float((ours - theirs).abs().max() / theirs.abs().max())}
        out['K%d' % K] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--n-wave', type=int, default=64, help='also time the first n wavenumbers only (0: not)')
    ap.add_argument('--skip-quarter-degree', action='store_true', help='leave out (8, 8, 4, 721, 1440)')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_spectrum: no HIP device (times are measured on the GPU or not at all)')
    dev = torch.device('cuda:0')
    out = {'reps': a.reps, 'device': torch.cuda.get_device_name(0)}
    out['ll181x360'] = _case((40, 32, 4, 181, 360), a.reps, a.n_wave, dev)
    torch.cuda.empty_cache()
    if not a.skip_quarter_degree:
        out['ll721x1440'] = _case((8, 8, 4, 721, 1440), a.reps, a.n_wave, dev)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
