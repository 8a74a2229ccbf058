#!/usr/bin/env python3
"""
Category scores of an ensemble on the device: what they cost.  One JSON line.

`ops.ensemble_category` (dlwpcs_ensemble_category) over ensembles laid out (member, lead x time, variable, face, height, width) on
C48 with 4 variables, fp32, M = 32, 128 and 320 members against Q = 2 and 9 thresholds per element, lead x time sized so that the
ensemble holds about --gb GB.  Per (M, Q): the rps-only call and the all-outputs call (prob, brier, rps, code) -- milliseconds
(device events, median of --reps calls after one warm-up call), GB/s over the bytes the call must move (M + 1 + Q fields read, one
written per output field), that rate over the device-to-device copy rate of the same ensemble in the same run (`of_copy`), the
plan, and the same numbers from a torch composition on the same tensors as the yardstick: per threshold a broadcast comparison
and a mean over the member axis, then the squares and their sum (its time, and the largest difference between the two rps fields).
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


def _torch_route(ens, y, thr, everything):
    prob = torch.stack([(ens <= thr[j]).to(torch.float32).mean(dim=0) for j in range(thr.shape[0])])
    obs = (y <= thr).to(torch.float32)
    brier = (prob - obs) ** 2
    rps = brier.sum(dim=0)
    if not everything:
        return rps
    M = ens.shape[0]
    return prob, brier, rps, (2.0 * M * prob + obs).round().to(torch.int32)


def _case(M, Q, gb, reps, dev):
    from DLWP import ops
    per_row = 4 * 6 * 48 * 48
    rows = max(1, int(round(gb * 1e9 / (4.0 * M * per_row))))
    gen = torch.Generator(device=dev).manual_seed(M + Q)
    y = 280.0 + 5.0 * torch.randn((rows, 4, 6, 48, 48), dtype=torch.float32, device=dev, generator=gen)
    ens = y + torch.randn((M,) + tuple(y.shape), dtype=torch.float32, device=dev, generator=gen)
    thr = torch.sort(280.0 + 5.0 * torch.randn((Q,) + tuple(y.shape), dtype=torch.float32, device=dev, generator=gen), dim=0).values
    n = y.numel()
    twin = torch.empty_like(ens)
    copy_ms = _time(lambda: twin.copy_(ens), reps)
    del twin
    copy_gbs = 2 * 4.0 * M * n / copy_ms / 1e6
    plan = ops.ensemble_category_plan(ens.shape, ens.stride(), thr.shape, thr.stride(), 0, 0, y.shape, y.stride(),
                                      ens_ptr=ens.data_ptr(), valid_ptr=y.data_ptr(), thr_ptr=thr.data_ptr())
    out = {'rows': rows, 'elements': n, 'ensemble_GB': round(4.0 * M * n / 1e9, 3), 'copy_GBs': round(copy_gbs, 1),
           'plan': {'q_class': plan['q_class'], 'vec': plan['vec'], 'valid': plan['valid'], 'thr': plan['thr']}}
    for tag, want in (('rps', ('rps',)), ('all', ('prob', 'brier', 'rps', 'code'))):
        ms = _time(lambda: ops.ensemble_category(ens, y, thr, want=want), reps)
        t_ms = _time(lambda: _torch_route(ens, y, thr, tag == 'all'), reps)
        fields_out = sum(Q if w in ('prob', 'brier', 'code') else 1 for w in want)
        gbs = 4.0 * n * (M + 1 + Q + fields_out) / ms / 1e6
        ours = ops.ensemble_category(ens, y, thr, want=('rps',))['rps']
        theirs = _torch_route(ens, y, thr, False)
        out[tag] = {'ms': round(ms, 3), 'GBs': round(gbs, 1), 'of_copy': round(gbs / copy_gbs, 3), 'torch_ms': round(t_ms, 3),
                    'torch_over_ours': round(t_ms / ms, 2), 'max_abs_diff': float((ours - theirs).abs().max())}
        del ours, theirs
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--gb', type=float, default=1.0, help='size of every ensemble')
    ap.add_argument('--members', type=int, nargs='+', default=[32, 128, 320])
    ap.add_argument('--thresholds', type=int, nargs='+', default=[2, 9])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_category: no HIP device (times are measured on the GPU or not at all)')
    dev = torch.device('cuda:0')
    out = {'reps': a.reps, 'device': torch.cuda.get_device_name(0)}
    for M in a.members:
        for Q in a.thresholds:
            out['M%d_Q%d' % (M, Q)] = _case(M, Q, a.gb, a.reps, dev)
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
