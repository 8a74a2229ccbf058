#!/usr/bin/env python3
"""
Spells along time on the device: what they cost.  One JSON line.

`ops.time_spell` (dlwpcs_time_spell) on a C48 series of 1024 times (time, variable-level, face, height, width), fp32, with as many
variable-levels as make about --gb GB (18 at 1 GB: 248 832 columns), and on a long thin series (--thin-columns columns, 10^5 rows)
that forces time slabs.  Per series: statistics only, length only and everything (position, length, statistics), each with a
scalar threshold, one threshold per column and one looked up per time from a 366-row table; the statistics and the length also
with every slab length forced, which is where the forms can be compared.  Per case: milliseconds (device events, median of --reps
calls after one warm-up call) and the plan.  Beside it, on the same tensors:
  - the torch route: c = x > h, `cummax` of the last false row index forward and on the flipped series, position and length by
    subtraction (several full-size temporaries), the statistics from them by reductions; checked equal to the kernel's integers;
  - the device-to-device copy rate measured in the same run, and what one read of the series, and one read plus the two int32
    writes, take at it.
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


def _torch_route(x, h, min_length, what):
    """(position, length, statistics) as torch gives them for x > h along dim 0; what: 'statistics', 'length' or 'all'"""
    T = x.shape[0]
    c = x > h
    t = torch.arange(T, device=x.device, dtype=torch.int32).view((T,) + (1,) * (x.dim() - 1))
    before = torch.where(c, torch.full_like(t, -1), t).cummax(dim=0).values
    after = (T - 1) - torch.where(c, torch.full_like(t, -1), (T - 1) - t).flip(0).cummax(dim=0).values.flip(0)
    n = after - before - 1
    q = c & (n >= min_length)
    ln = torch.where(q, n, torch.zeros_like(n))
    if what == 'length':
        return None, ln, None
    pos = torch.where(q, t - before, torch.zeros_like(n))
    longest = ln.max(dim=0)
    parts = [(~(torch.isnan(x) | torch.isnan(h))).expand_as(x).sum(0), c.sum(0), (pos == 1).sum(0), q.sum(0), longest.values,
             torch.where(longest.values > 0, longest.indices, torch.full_like(longest.indices, -1))]
    stats = torch.stack([v.to(torch.int32) for v in parts])
    return (None, None, stats) if what == 'statistics' else (pos, ln, stats)


def _thresholds(x, gen):
    """{name: (threshold for ops.time_spell, its index, the (T, ...) or broadcast h of the torch route)}"""
    T, dev = x.shape[0], x.device
    col = 280.0 + torch.randn((1,) + tuple(x.shape[1:]), dtype=torch.float32, device=dev, generator=gen)
    table = 280.0 + torch.randn((366,) + tuple(x.shape[1:]), dtype=torch.float32, device=dev, generator=gen)
    idx = (torch.arange(T, device=dev) % 366).to(torch.int32)
    return {'scalar': (280.0, None, torch.full((), 280.0, device=dev)), 'column': (col, None, col), 'table366': (table, idx, (table, idx))}


def _series(ops, x, gen, reps, min_length, slabs, torch_route=True):
    rec = {}
    wants = {'statistics': dict(statistics=True), 'length': dict(length=True, statistics=False),
             'all': dict(position=True, length=True, statistics=True)}
    for tname, (thr, idx, h) in _thresholds(x, gen).items():
        for wname, want in wants.items():
            per_row = wname != 'statistics'
            r = {}
            for slab in [None] + (slabs[wname] if tname == 'scalar' else []):
                plan = ops.time_spell_plan(x.shape, x.stride(), per_row=per_row, slab_rows=slab)
                ms = _time(lambda: ops.time_spell(x, thr, idx, min_length=min_length, slab_rows=slab, **want), reps)
                r['chosen' if slab is None else 'slab%d' % slab] = {'ms': round(ms, 3), 'plan': plan}
            if torch_route:
                hh = h[0].index_select(0, h[1].long()) if isinstance(h, tuple) else h       # (the looked-up series laid out: outside the timing)
                r['torch_route_ms'] = round(_time(lambda: _torch_route(x, hh, min_length, wname), reps), 3)
                ours = ops.time_spell(x, thr, idx, min_length=min_length, **want)
                ours = ours if isinstance(ours, tuple) else (ours,)
                theirs = [v for v in _torch_route(x, hh, min_length, wname) if v is not None]
                r['equal_to_torch'] = all(bool((a.reshape(b.shape) == b).all()) for a, b in zip(ours, theirs))
                r['torch_over_chosen'] = round(r['torch_route_ms'] / r['chosen']['ms'], 2)
                del ours, theirs, hh
                torch.cuda.empty_cache()
            rec['%s_%s' % (wname, tname)] = r
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--gb', type=float, default=1.0, help='size of the C48 series')
    ap.add_argument('--thin-columns', type=int, default=4)
    ap.add_argument('--min-length', type=int, default=3)
    ap.add_argument('--no-torch', action='store_true', help='skip the torch route')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_spell: no HIP device (times are measured on the GPU or not at all)')
    from DLWP import ops
    dev = torch.device('cuda:0')
    T = 1024
    nvar = max(1, int(round(a.gb * 1e9 / (4.0 * T * 6 * 48 * 48))))
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((T, nvar, 6, 48, 48), dtype=torch.float32, device=dev, generator=gen)
    for t in range(1, T):                                                   # red noise: spells of a few days
        x[t].mul_(0.6).add_(x[t - 1], alpha=0.8)
    x.add_(280.0)
    nbytes = 4.0 * x.numel()
    twin = torch.empty_like(x)
    copy_ms = _time(lambda: twin.copy_(x), a.reps)
    del twin
    copy_gbs = 2 * nbytes / copy_ms / 1e6
    out = {'reps': a.reps, 'device': torch.cuda.get_device_name(0), 'min_length': a.min_length, 'copy_GBs': round(copy_gbs, 1),
           'c48': {'steps': T, 'columns': nvar * 6 * 48 * 48, 'series_GB': round(nbytes / 1e9, 3), 'one_read_ms': round(nbytes / copy_gbs / 1e6, 3),
                   'read_and_two_writes_ms': round(3 * nbytes / copy_gbs / 1e6, 3)}}
    out['c48'].update(_series(ops, x, gen, a.reps, a.min_length, {'statistics': [1024, 256, 128], 'length': [1024, 512, 256, 128, 32],
                                                                   'all': [1024, 256]}, not a.no_torch))
    del x
    torch.cuda.empty_cache()
    Tt = 100000
    thin = torch.randn((Tt, a.thin_columns), dtype=torch.float32, device=dev, generator=gen)
    thin = 280.0 + torch.where(thin.cumsum(0).sin() > -0.5, thin.abs(), -thin.abs())
    out['thin'] = {'steps': Tt, 'columns': a.thin_columns}
    out['thin'].update(_series(ops, thin, gen, a.reps, a.min_length, {'statistics': [Tt // 32 * 32 + 32, 4096, 1024, 256],
                                                                       'length': [1024, 256, 64, 32], 'all': [1024, 32]}, not a.no_torch))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
