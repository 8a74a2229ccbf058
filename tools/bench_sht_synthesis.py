#!/usr/bin/env python3
"""
Spherical-harmonic analysis, synthesis and filtering on the device: what they cost.  One JSON line.

`ops.spherical_analysis` (dlwpcs_sht_analysis), `ops.spherical_synthesis` (dlwpcs_sht_synthesis) and their chain with a truncation
response (what verify.spherical_filter launches), over --fields fields (default 512 and 4096) on clenshaw-curtis grids: 181 x 360
at T = 90 and 361 x 720 at T = 180.  Per case and operation: milliseconds (device events, median of --reps calls after one warm-up
call) and microseconds per field; the same result from a torch expression on the same tensors as the yardstick -- torch.fft.rfft /
irfft and one torch.einsum per order m with the same fp32 tables -- with its time and the largest difference between the two
results relative to the largest value; the time of a device copy of the grid bytes; the peak device memory of either route.
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


def _torch_analysis(x, tables, T, L):
    """rfft, one complex einsum per order with the weighted fp32 table: complex64 (fields, rows)"""
    X = torch.fft.rfft(x, dim=-1)[..., :T + 1] / L
    return torch.cat([torch.einsum('ni,fi->fn', tables[m].to(X.dtype), X[..., m]) for m in range(T + 1)], dim=-1)


def _torch_synthesis(coef, resp, starts, ptables, T, nlat, L):
    """one complex einsum per order with the unweighted fp32 table, irfft: float32 (fields, nlat, L)"""
    G = torch.zeros((coef.shape[0], nlat, L // 2 + 1), dtype=coef.dtype, device=coef.device)
    for m in range(T + 1):
        a = coef[:, starts[m]:starts[m] + T + 1 - m]
        if resp is not None:
            a = a * resp[m:]
        G[..., m] = torch.einsum('ni,fn->fi', ptables[m].to(coef.dtype), a)
    return torch.fft.irfft(G * L, n=L, dim=-1)


def _rel(a, b):
    a, b = (torch.view_as_real(t) if t.is_complex() else t for t in (a, b))
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def _case(nlat, L, fields, reps, dev):
    from DLWP import ops
    from DLWP.remap import spharm
    tr = spharm.SphericalTransform(np.linspace(90., -90., nlat), L)
    T = tr.truncation
    gen = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn((fields, nlat, L), dtype=torch.float32, device=dev, generator=gen)
    _, table = tr.device_tables(dev)
    _, ptable = tr.device_synthesis_tables(dev)
    starts = [spharm.packed_row(m, m, T) for m in range(T + 1)]
    tables = [table[s:s + T + 1 - m, :nlat].contiguous() for m, s in enumerate(starts)]
    ptables = [ptable[s:s + T + 1 - m, :nlat].contiguous() for m, s in enumerate(starts)]
    resp = torch.from_numpy(spharm.truncation_response(T, T // 4).astype(np.float32)).to(dev)
    coef = ops.spherical_analysis(x, tr)
    out = torch.empty_like(x)
    res = {'nlat': nlat, 'L': L, 'T': T, 'fields': fields}
    routes = {
        'analysis': (lambda: ops.spherical_analysis(x, tr), lambda: _torch_analysis(x, tables, T, L)),
        'synthesis': (lambda: ops.spherical_synthesis(coef, tr, out=out),
                      lambda: _torch_synthesis(coef, None, starts, ptables, T, nlat, L)),
        'filter': (lambda: ops.spherical_synthesis(ops.spherical_analysis(x, tr), tr, resp, out=out),
                   lambda: _torch_synthesis(_torch_analysis(x, tables, T, L), resp, starts, ptables, T, nlat, L)),
    }
    for name, (ours, theirs) in routes.items():
        ms, peak = _time(ours, reps)
        t_ms, t_peak = _time(theirs, reps)
        res[name] = {'ms': round(ms, 3), 'us_per_field': round(1e3 * ms / fields, 3), 'torch_ms': round(t_ms, 3),
                     'torch_over_ours': round(t_ms / ms, 2), 'peak_MB': round(peak / 1e6, 1), 'torch_peak_MB': round(t_peak / 1e6, 1),
                     'max_rel_diff': _rel(ours().clone(), theirs())}
    c_ms, _ = _time(lambda: out.copy_(x), reps)
    res['copy_ms'] = round(c_ms, 3)
    res['copy_GBs'] = round(8.0 * nlat * L * fields / c_ms / 1e6, 1)
    for name in routes:
        res[name]['over_copy'] = round(res[name]['ms'] / c_ms, 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--fields', type=int, nargs='+', default=[512, 4096])
    ap.add_argument('--skip-half-degree', action='store_true', help='leave out 361 x 720 at T = 180')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_sht_synthesis: no HIP device (times are measured on the GPU or not at all)')
    dev = torch.device('cuda:0')
    out = {'reps': a.reps, 'device': torch.cuda.get_device_name(0), 'cases': []}
    for nlat, L in [(181, 360)] + ([] if a.skip_half_degree else [(361, 720)]):
        for fields in a.fields:
            out['cases'].append(_case(nlat, L, fields, a.reps, dev))
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
