#!/usr/bin/env python3
"""
Ensemble scores on the device: what they cost.  One JSON line.

`ops.ensemble_stats` (dlwpcs_ensemble_stats) over ensembles laid out (member, lead x time, variable, face, height, width) on C48
with 4 variables, fp32, M = 8, 32 and 128 members, lead x time sized so that the ensemble holds about --gb GB.  Per M: the
all-outputs call (mean, spread, crps, rank) and the crps-only call -- milliseconds (device events, median of --reps calls after one
warm-up call), GB/s over the bytes the call must move ((M + 1) fields read, one written per output), that rate over the
device-to-device copy rate of the same ensemble in the same run (`of_copy`, as tools/bench_missing.py reports it), and the same
numbers from a torch composition on the same tensors as the yardstick: `torch.sort` along the member axis plus the weighted sum
sum_i (2 i - M - 1) x_(i), mean |x - y|, mean, std and a comparison count (its time, and the largest difference between the two
crps fields relative to the largest value).
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


def _torch_route(ens, y, everything):
    M = ens.shape[0]
    xs = torch.sort(ens, dim=0).values
    coef = (2.0 * torch.arange(1, M + 1, device=ens.device, dtype=torch.float32) - M - 1).view((M,) + (1,) * (ens.dim() - 1))
    crps = (ens - y).abs().mean(dim=0) - (coef * xs).sum(dim=0) / float(M * M)
    if not everything:
        return crps
    return crps, ens.mean(dim=0), ens.std(dim=0), (ens < y).sum(dim=0, dtype=torch.int32)


def _case(M, gb, reps, dev):
    from DLWP import ops
    per_row = 4 * 6 * 48 * 48
    rows = max(1, int(round(gb * 1e9 / (4.0 * M * per_row))))
    gen = torch.Generator(device=dev).manual_seed(M)
    y = 280.0 + 5.0 * torch.randn((rows, 4, 6, 48, 48), dtype=torch.float32, device=dev, generator=gen)
    ens = y + torch.randn((M,) + tuple(y.shape), dtype=torch.float32, device=dev, generator=gen)
    n = y.numel()
    twin = torch.empty_like(ens)
    copy_ms = _time(lambda: twin.copy_(ens), reps)
    del twin
    copy_gbs = 2 * 4.0 * M * n / copy_ms / 1e6
    plan = ops.ensemble_plan(ens.shape, ens.stride(), 0, y.shape, y.stride(), ens_ptr=ens.data_ptr(), valid_ptr=y.data_ptr())
    out = {'rows': rows, 'elements': n, 'ensemble_GB': round(4.0 * M * n / 1e9, 3), 'copy_GBs': round(copy_gbs, 1),
           'plan': {'m_class': plan['m_class'], 'vec': plan['vec'], 'lds': plan['lds']}}
    for tag, want in (('all', ('mean', 'spread', 'crps', 'rank')), ('crps', ('crps',))):
        ms = _time(lambda: ops.ensemble_stats(ens, y, want=want), reps)
        t_ms = _time(lambda: _torch_route(ens, y, tag == 'all'), reps)
        gbs = 4.0 * n * (M + 1 + len(want)) / ms / 1e6
        ours = ops.ensemble_stats(ens, y, want=('crps',))['crps']
        theirs = _torch_route(ens, y, False)
        out[tag] = {'ms': round(ms, 3), 'GBs': round(gbs, 1), 'of_copy': round(gbs / copy_gbs, 3), 'torch_ms': round(t_ms, 3),
                    'torch_over_ours': round(t_ms / ms, 2), 'max_rel_diff': float((ours - theirs).abs().max() / theirs.abs().max())}
        del ours, theirs
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--gb', type=float, default=1.0, help='size of every ensemble')
    ap.add_argument('--members', type=int, nargs='+', default=[8, 32, 128])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_ensemble: no HIP device (times are measured on the GPU or not at all)')
    dev = torch.device('cuda:0')
    out = {'reps': a.reps, 'device': torch.cuda.get_device_name(0)}
    for M in a.members:
        out['M%d' % M] = _case(M, a.gb, a.reps, dev)
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
