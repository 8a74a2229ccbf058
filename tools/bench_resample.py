#!/usr/bin/env python3
"""
Block-bootstrap means on the device: what they cost.  One JSON line.

`ops.row_resample` (dlwpcs_row_resample) on a C48 series of 1024 times (time, variable-level, face, height, width), fp32, with as
many variable-levels as make about --gb GB (18 at 1 GB: 248 832 columns): B = 200 and 1000 resamples in blocks of L = 1 and 8, on
a complete series and with 1 % NaN, in each form the kernel can run (staged as the planner chooses it, direct forced).  Per case:
milliseconds (device events, median of --reps calls after one warm-up call) and the plan.  Beside it, on the same tensors and the
same draw table:
  - the route a user has without the kernel: `ops.group_mean` with one group per resample (B x T row indices), which reads the
    series B times;
  - the torch route: `index_select` of the drawn rows and `nanmean`, two resamples a chunk (the gathered rows are a temporary of
    the chunk's size); timed on the first --torch-resamples resamples and scaled to B, which the record says;
  - the device-to-device copy rate measured in the same run, and the time one read of the series takes at it.
The largest difference of the kernel's result from the group_mean route is recorded too (the two add their float64 terms in
different orders and round to float32 once: at most one float32 rounding, and 0 where the two float64 sums round alike).  Then the
small case: 40 columns under B = 10 000 (two column tiles of 32), where the resamples of a column tile are cut into ranges -- as
the planner chooses, unsplit, and direct.  And the series seen as 2048 rows of half the columns, past the staged cap, where the
planner itself takes the direct form (B = 200, with the 1 % NaN).
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


def _rows(st, T, L):
    """(B, n_draw) drawn rows of a draw table with n_draw = T"""
    r = (st[:, :, None].astype(np.int64) + np.arange(L)[None, None, :]) % T
    return r.reshape(st.shape[0], -1)[:, :T]


def _torch_route(x, rows_d, chunk=2):
    out = []
    T = x.shape[0]
    for b in range(0, rows_d.shape[0], chunk):
        idx = rows_d[b:b + chunk].reshape(-1)
        g = x.index_select(0, idx).view((-1, T) + tuple(x.shape[1:]))
        out.append(g.nanmean(dim=1))
    return torch.cat(out)


def _case(ops, x, B, L, reps, torch_resamples, forms, seed=0):
    from DLWP import verify as V
    T = int(x.shape[0])
    dev = x.device
    st = V.bootstrap_starts(T, B, L, seed=seed)
    st_d = torch.from_numpy(st).to(dev)
    nb = st.shape[1]
    rec = {}
    ours = None
    for name, kw in forms:
        plan = ops.row_resample_plan(x.shape, x.stride(), B, nb, L, **kw)
        ms = _time(lambda: ops.row_resample(x, st_d, block_length=L, **kw), reps)
        rec[name] = {'ms': round(ms, 3), 'plan': plan}
        if ours is None:
            ours = ops.row_resample(x, st_d, block_length=L, **kw)
    rows = _rows(st, T, L)
    gs, ri = np.arange(B + 1, dtype=np.int64) * T, rows.reshape(-1)
    gm_ms = _time(lambda: ops.group_mean(x, gs, ri, row_axis=0), reps)
    ref = ops.group_mean(x, gs, ri, row_axis=0)
    diff = ((ours - ref).abs() / ref.nan_to_num(0.0).abs().max()).nan_to_num(0.0, 0.0, 0.0)
    rec['group_mean_route'] = {'ms': round(gm_ms, 3), 'max_rel_diff': float(diff.max())}
    del ref, diff, ours
    torch.cuda.empty_cache()
    if torch_resamples:
        nt = min(B, torch_resamples)
        rows_d = torch.from_numpy(rows[:nt]).to(dev)
        t_ms = _time(lambda: _torch_route(x, rows_d), reps)
        rec['torch_route'] = {'ms': round(t_ms * B / nt, 3), 'timed_resamples': nt, 'scaled_to': B}
        del rows_d
        torch.cuda.empty_cache()
    best = min(v['ms'] for k, v in rec.items() if 'plan' in v)
    rec['group_mean_over_best'] = round(gm_ms / best, 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--gb', type=float, default=1.0, help='size of the series')
    ap.add_argument('--torch-resamples', type=int, default=50, help='resamples the torch route is timed on (0: skip it)')
    ap.add_argument('--quick', action='store_true', help='B = 200 only')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_resample: no HIP device (times are measured on the GPU or not at all)')
    from DLWP import ops
    dev = torch.device('cuda:0')
    T = 1024
    nvar = max(1, int(round(a.gb * 1e9 / (4.0 * T * 6 * 48 * 48))))
    shape = (T, nvar, 6, 48, 48)
    gen = torch.Generator(device=dev).manual_seed(1)
    x = 280.0 + 5.0 * torch.randn(shape, dtype=torch.float32, device=dev, generator=gen)
    nbytes = 4.0 * x.numel()
    twin = torch.empty_like(x)
    copy_ms = _time(lambda: twin.copy_(x), a.reps)
    del twin
    copy_gbs = 2 * nbytes / copy_ms / 1e6
    out = {'reps': a.reps, 'device': torch.cuda.get_device_name(0), 'steps': T, 'columns': nvar * 6 * 48 * 48, 'series_GB': round(nbytes / 1e9, 3),
           'copy_GBs': round(copy_gbs, 1), 'one_read_ms': round(nbytes / copy_gbs / 1e6, 3)}
    forms = (('staged', {}), ('direct', {'form': 'direct'}))
    for missing in (False, True):
        if missing:
            x = torch.where(torch.rand(shape, device=dev, generator=gen) < 0.01, torch.full_like(x, float('nan')), x)
        for B in ((200,) if a.quick else (200, 1000)):
            for L in (1, 8):
                out['B%d_L%d%s' % (B, L, '_nan' if missing else '')] = _case(ops, x, B, L, a.reps, a.torch_resamples, forms)
    # past the staged cap, where the planner itself takes the direct form: the same memory as 2048 rows of half the columns
    long = x.reshape(2 * T, -1)
    for L in (1, 8):
        out['rows2048_B200_L%d_nan' % L] = _case(ops, long, 200, L, a.reps, 0, (('chosen', {}),))
    del x, long
    torch.cuda.empty_cache()
    small = 280.0 + 5.0 * torch.randn((T, 40), dtype=torch.float32, device=dev, generator=gen)
    forms = (('staged', {}), ('staged_unsplit', {'splits': 1}), ('direct', {'form': 'direct'}), ('direct_unsplit', {'form': 'direct', 'splits': 1}))
    for L in (1, 8):
        out['small_40_columns_B10000_L%d' % L] = _case(ops, small, 10000, L, a.reps, 0, forms)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
