#!/usr/bin/env python3
"""
Spherical-harmonic spectra on the device: what they cost.  One JSON line.

`ops.spherical_spectrum` (dlwpcs_sht_spectrum), pair form, per field (nothing averaged), over --fields fields (default 512 and
4096) on clenshaw-curtis grids: 181 x 360 at T = 90 and 361 x 720 at T = 180.  Per case: milliseconds (device events, median of
--reps calls after one warm-up call), the same result from a torch expression on the same tensors as the yardstick -- torch.fft.rfft,
one torch.einsum per order m with the same Legendre table, torch reductions -- with its time and the largest difference between
the two results relative to the largest value, the time of a device copy of the input bytes, the algorithmic flops of the two
stages (stage A: 2 L 2 (T + 1) per latitude row; stage B: 2 nlat 2 per coefficient (m, n)), and the peak device memory of either
route.  The share of each stage is read from a kernel trace of this tool (the two kernels are sht_fourier_kernel and
sht_legendre_kernel), not measured here.
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


def _torch_route(f, v, tables, T, L):
    """the yardstick: rfft, one einsum per order with the same fp32 table, powers summed over m; (3, fields, T + 1)"""
    F = torch.fft.rfft(f, dim=-1)[..., :T + 1] / L
    V = torch.fft.rfft(v, dim=-1)[..., :T + 1] / L
    out = torch.zeros((3, f.shape[0], T + 1), dtype=torch.float64, device=f.device)
    for m in range(T + 1):
        t = tables[m]                                                   # (T + 1 - m, nlat)
        fr, fi = torch.einsum('ni,fi->fn', t, F[..., m].real), torch.einsum('ni,fi->fn', t, F[..., m].imag)
        vr, vi = torch.einsum('ni,fi->fn', t, V[..., m].real), torch.einsum('ni,fi->fn', t, V[..., m].imag)
        c = 1.0 if m == 0 else 2.0
        out[0, :, m:] += c * (fr * fr + fi * fi)
        out[1, :, m:] += c * (vr * vr + vi * vi)
        out[2, :, m:] += c * (fr * vr + fi * vi)
    return out


def _case(nlat, L, fields, reps, dev):
    from DLWP import ops
    from DLWP.remap import spharm
    tr = spharm.SphericalTransform(np.linspace(90., -90., nlat), L)
    T = tr.truncation
    gen = torch.Generator(device=dev).manual_seed(3)
    f = torch.randn((fields, nlat, L), dtype=torch.float32, device=dev, generator=gen)
    v = torch.roll(f, 2, dims=-1) + 0.5 * torch.randn((fields, nlat, L), dtype=torch.float32, device=dev, generator=gen)
    _, table = tr.device_tables(dev)
    tables = [table[spharm.packed_row(m, m, T):spharm.packed_row(m, m, T) + T + 1 - m, :nlat].contiguous() for m in range(T + 1)]
    ms, peak = _time(lambda: ops.spherical_spectrum(f, v, transform=tr), reps)
    t_ms, t_peak = _time(lambda: _torch_route(f, v, tables, T, L), reps)
    dst = torch.empty_like(f)
    c_ms, _ = _time(lambda: (dst.copy_(f), dst.copy_(v)), reps)
    ours = ops.spherical_spectrum(f, v, transform=tr).double()
    theirs = _torch_route(f, v, tables, T, L)
    flops_a = 2.0 * L * 2 * (T + 1) * nlat * fields * 2
    flops_b = 2.0 * nlat * 2 * ((T + 1) * (T + 2) // 2) * fields * 2
    return {'nlat': nlat, 'L': L, 'T': T, 'fields': fields, 'ms': round(ms, 3), 'torch_ms': round(t_ms, 3),
            'torch_over_ours': round(t_ms / ms, 2), 'copy_ms': round(c_ms, 3), 'ours_over_copy': round(ms / c_ms, 2),
            'GBs_in': round(8.0 * nlat * L * fields / ms / 1e6, 1), 'stage_a_GF': round(flops_a / 1e9, 2),
            'stage_b_GF': round(flops_b / 1e9, 2), 'TFs': round((flops_a + flops_b) / ms / 1e9, 2),
            'peak_MB': round(peak / 1e6, 1), 'torch_peak_MB': round(t_peak / 1e6, 1),
            'max_rel_diff': float((ours - theirs).abs().max() / theirs.abs().max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--fields', type=int, nargs='+', default=[512, 4096])
    ap.add_argument('--skip-half-degree', action='store_true', help='leave out 361 x 720 at T = 180')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_sht: no HIP device (times are measured on the GPU or not at all)')
    dev = torch.device('cuda:0')
    out = {'reps': a.reps, 'device': torch.cuda.get_device_name(0), 'cases': []}
    for nlat, L in [(181, 360)] + ([] if a.skip_half_degree else [(361, 720)]):
        for fields in a.fields:
            out['cases'].append(_case(nlat, L, fields, a.reps, dev))
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
