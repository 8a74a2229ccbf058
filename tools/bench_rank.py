#!/usr/bin/env python3
"""
Rank statistics along time on the device: what they cost.  One JSON line.

`ops.time_rank` (dlwpcs_time_rank) on a C48 series of 1024 times (time, variable-level, face, height, width), fp32, with as many
variable-levels as make about --gb GB (18 at 1 GB: 248 832 columns): the Mann-Kendall statistics (trend form), the Kendall pair
statistics against a second series of the same shape, and the ranks alone; and a direct-form point past the staged cap with few
columns (--thin-rows rows, --thin-columns columns).  Per case: milliseconds (device events, median of --reps calls after one
warm-up call) and the plan.  Beside it:
  - the torch route a user would write today, on a slice of --torch-columns columns and scaled to the whole series by the column
    count (it is linear in the columns and takes seconds on the whole): for S a loop over i of sign(x[i+1:] - x[i]).sum(0); for
    the ranks a double argsort, which gives ordinal ranks and no mid-ranks: it answers an easier question;
  - a bound: the pairs a launch visits x its columns x the vector instructions the kernel's inner loop spends per pair (read from
    the ISA) over the device's vector lane rate (256 CUs x 4 SIMDs x 32 lanes a cycle at --ghz), and the fraction of
    it that the measured time reaches.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'dlwp-cs_amd')]

import numpy as np   # noqa: E402
import torch         # noqa: E402

# vector instructions per pair in the unrolled inner loops of csrc/rank.hip as compiled for gfx950 (a compare and an add-with-carry
# per count; the pair form spends its mask logic on the scalar unit): see DESIGN.md
VALU_PER_PAIR = {'trend_stats': 6.0, 'pair_stats': 11.2, 'ranks': 4.3}
LANES_PER_CYCLE = 256 * 4 * 32


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


def _torch_s(x):
    T = x.shape[0]
    s = torch.zeros(x.shape[1:], dtype=torch.float32, device=x.device)
    for i in range(T - 1):
        s += torch.sign(x[i + 1:] - x[i]).sum(0)
    return s


def _torch_ranks(x):
    return x.argsort(dim=0).argsort(dim=0)


def _bound_ms(kind, pairs, columns, ghz):
    return pairs * columns * VALU_PER_PAIR[kind] / (LANES_PER_CYCLE * ghz * 1e9) * 1e3


def _case(kind, fn, plan, pairs, columns, reps, ghz):
    ms = _time(fn, reps)
    bound = _bound_ms(kind, pairs, columns, ghz)
    return {'ms': round(ms, 3), 'plan': plan, 'bound_ms': round(bound, 3), 'fraction_of_bound': round(bound / ms, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--gb', type=float, default=1.0, help='size of the C48 series')
    ap.add_argument('--thin-rows', type=int, default=4096)
    ap.add_argument('--thin-columns', type=int, default=64)
    ap.add_argument('--torch-columns', type=int, default=6 * 48 * 48)
    ap.add_argument('--ghz', type=float, default=2.4)
    ap.add_argument('--no-torch', action='store_true', help='skip the torch route')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_rank: no HIP device (times are measured on the GPU or not at all)')
    from DLWP import ops
    dev = torch.device('cuda:0')
    T = 1024
    nvar = max(1, int(round(a.gb * 1e9 / (4.0 * T * 6 * 48 * 48))))
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((T, nvar, 6, 48, 48), dtype=torch.float32, device=dev, generator=gen)
    cols = nvar * 6 * 48 * 48
    tri, full = T * (T - 1) // 2, T * T
    out = {'reps': a.reps, 'device': torch.cuda.get_device_name(0), 'ghz': a.ghz, 'valu_per_pair': VALU_PER_PAIR,
           'c48': {'steps': T, 'columns': cols, 'series_GB': round(4.0 * x.numel() / 1e9, 3)}}
    c = out['c48']
    c['mann_kendall_stats'] = _case('trend_stats', lambda: ops.time_rank(x), ops.time_rank_plan(x.shape, x.stride()), tri, cols,
                                    a.reps, a.ghz)
    c['ranks'] = _case('ranks', lambda: ops.time_rank(x, ranks=True, stats=False),
                       ops.time_rank_plan(x.shape, x.stride(), per_row=True), full, cols, a.reps, a.ghz)
    if not a.no_torch:
        k = min(a.torch_columns, x[0].numel())
        xs = x.reshape(T, -1)[:, :k].contiguous()
        scale = cols / float(k)
        s_ms, r_ms = _time(lambda: _torch_s(xs), 1), _time(lambda: _torch_ranks(xs), a.reps)
        st = ops.time_rank(xs)
        c['torch_route'] = {'columns_timed': k, 'S_loop_ms_scaled': round(s_ms * scale, 1), 'double_argsort_ms_scaled': round(r_ms * scale, 1),
                            'note': 'the double argsort gives ordinal ranks, no mid-ranks',
                            'S_equal_to_torch': bool(((st[1] - st[2]).reshape(-1).to(torch.float32) == _torch_s(xs).reshape(-1)).all())}
        c['torch_S_over_kernel'] = round(s_ms * scale / c['mann_kendall_stats']['ms'], 1)
        c['torch_argsort_over_kernel'] = round(r_ms * scale / c['ranks']['ms'], 2)
        del xs, st
    y = torch.randn(x.shape, dtype=torch.float32, device=dev, generator=gen)
    c['kendall_pair_stats'] = _case('pair_stats', lambda: ops.time_rank(x, y), ops.time_rank_plan(x.shape, x.stride(), kind='pair'),
                                    tri, cols, a.reps, a.ghz)
    del x, y
    torch.cuda.empty_cache()
    Tt, Et = a.thin_rows, a.thin_columns
    thin = torch.randn((Tt, Et), dtype=torch.float32, device=dev, generator=gen)
    out['thin'] = {'steps': Tt, 'columns': Et}
    if ops.time_rank_plan(thin.shape, thin.stride())['form'] != 'direct':
        raise SystemExit('bench_rank: --thin-rows %d fits a staged tile; the thin case is the direct form (more than %d rows)' % (Tt, ops.RANK_STAGE_ROWS[-1]))
    out['thin']['mann_kendall_stats'] = _case('trend_stats', lambda: ops.time_rank(thin), ops.time_rank_plan(thin.shape, thin.stride()),
                                              Tt * (Tt - 1) // 2, Et, a.reps, a.ghz)
    out['thin']['ranks'] = _case('ranks', lambda: ops.time_rank(thin, ranks=True, stats=False),
                                 ops.time_rank_plan(thin.shape, thin.stride(), per_row=True), Tt * Tt, Et, a.reps, a.ghz)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
