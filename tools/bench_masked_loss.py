#!/usr/bin/env python3
"""
What the masked losses and the missing-value fill cost.  One JSON line.

  * loss: at the headline output shape (32, 6, 48, 48, 4), bf16 prediction against the fp32 target, with the gradient:
    `dlwpcs_loss_fwd_bwd` (plain 'mse') and `dlwpcs_loss_masked_fwd_bwd` under both normalisations, with no hole and with 30 % of the
    targets NaN.  `over_plain` is the ratio of the medians.  DLWPCS_NORM_ALL moves the plain call's bytes (y, t read, dy written);
    DLWPCS_NORM_VALID reads y and t a second time in its gradient launch.
  * fill: `dlwpcs_fill_missing` in place on the bf16 predictor batch (32, 6, 48, 48, --channels), 30 % NaN in two of the channels,
    against a device-to-device copy of the same bytes in the same run (`over_copy`: both read and write every byte once).
Each timing is --calls calls captured in one hipGraph and replayed between two device events (a call is two or three launches
of a few microseconds: enqueued one by one the host would be what is timed); the variants are timed in interleaved rounds and
the median over --rounds is reported, in microseconds per call.

    python tools/bench_masked_loss.py [--calls 200] [--rounds 7] [--channels 10]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'dlwp-cs_amd')]

import numpy as np   # noqa: E402
import torch         # noqa: E402


def _graph(fn, calls):
    """fn() `calls` times in one captured graph"""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def _rounds(graphs, calls, rounds):
    """{name: median microseconds per call}, the graphs replayed in interleaved rounds"""
    us = {k: [] for k in graphs}
    for _ in range(rounds):
        for name, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / calls)
    return {k: float(np.median(v)) for k, v in us.items()}, {k: [round(x, 3) for x in v] for k, v in us.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--channels', type=int, default=10, help='channels of the predictor batch of the fill')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_masked_loss: no HIP device (times are measured on the GPU or not at all)')
    from DLWP import _native as nat
    lib = nat.lib()
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(1)
    shape = (32, 6, 48, 48, 4)
    t = torch.randn(shape, dtype=torch.float32, device=dev, generator=gen)
    y = (t + 0.5 * torch.randn(shape, dtype=torch.float32, device=dev, generator=gen)).to(torch.bfloat16)
    th = t.clone()
    th[torch.rand(shape, device=dev, generator=gen) < 0.3] = float('nan')
    dy = torch.empty_like(y)
    out = torch.zeros(2, dtype=torch.float32, device=dev)
    scratch = torch.empty(lib.dlwpcs_loss_scratch_bytes(), dtype=torch.uint8, device=dev)
    n = y.numel()
    L = nat.LossDesc()
    L.kind, L.loss_weight, L.overwrite = nat.LOSS_MSE, 1.0, 1
    tag = nat.BF16 | nat.MSE_TARGET_F32
    res = {'device': torch.cuda.get_device_name(0), 'calls': a.calls, 'rounds': a.rounds, 'shape': list(shape)}

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        def plain(tt):
            return lambda: nat.check(lib.dlwpcs_loss_fwd_bwd(ctypes.byref(L), y.data_ptr(), tt.data_ptr(), dy.data_ptr(), out.data_ptr(), n,
                                                             tag, scratch.data_ptr(), nat.stream_ptr()), 'dlwpcs_loss_fwd_bwd')

        def masked(tt, norm):
            return lambda: nat.check(lib.dlwpcs_loss_masked_fwd_bwd(ctypes.byref(L), y.data_ptr(), tt.data_ptr(), norm, dy.data_ptr(),
                                                                    out.data_ptr(), None, n, tag, scratch.data_ptr(), nat.stream_ptr()),
                                     'dlwpcs_loss_masked_fwd_bwd')
        graphs = {'plain': _graph(plain(t), a.calls)}
        for holes, tt in (('0pct', t), ('30pct', th)):
            graphs['all_' + holes] = _graph(masked(tt, nat.NORM_ALL), a.calls)
            graphs['valid_' + holes] = _graph(masked(tt, nat.NORM_VALID), a.calls)
        med, raw = _rounds(graphs, a.calls, a.rounds)
        # bytes the algorithm moves: y (2 B) and t (4 B) read, dy (2 B) written; NORM_VALID reads y and t twice
        moved = {k: n * (14 if k.startswith('valid') else 8) for k in med}
        res['loss'] = {k: {'us': round(v, 3), 'over_plain': round(v / med['plain'], 3), 'GB_per_s': round(moved[k] / v * 1e-3, 1)}
                       for k, v in med.items()}
        res['loss_rounds_us'] = raw

        # ---- fill against a copy of the same bytes ----
        pshape = (32, 6, 48, 48, a.channels)
        x = torch.randn(pshape, dtype=torch.float32, device=dev, generator=gen).to(torch.bfloat16)
        hole = torch.rand(pshape[:-1], device=dev, generator=gen) < 0.3
        x[..., 1][hole] = float('nan')
        x[..., a.channels - 1][hole] = float('nan')
        work, dst = x.clone(), torch.empty_like(x)
        fill = torch.arange(a.channels, dtype=torch.float32, device=dev)
        nx = x.numel()

        def fill_call():
            # (after the first call of a graph nothing is NaN any more: the pass reads and writes every byte either way)
            nat.check(lib.dlwpcs_fill_missing(work.data_ptr(), nat.BF16, nx, fill.data_ptr(), 1, a.channels, nat.stream_ptr()),
                      'dlwpcs_fill_missing')
        fgraphs = {'fill': _graph(fill_call, a.calls), 'copy': _graph(lambda: dst.copy_(x), a.calls)}
        work.copy_(x)
        med, raw = _rounds(fgraphs, a.calls, a.rounds)
        res['fill'] = {'shape': list(pshape), 'dtype': 'bf16', 'fill_us': round(med['fill'], 3), 'copy_us': round(med['copy'], 3),
                       'over_copy': round(med['fill'] / med['copy'], 3), 'GB_per_s': round(2 * nx * 2 / med['fill'] * 1e-3, 1)}
        res['fill_rounds_us'] = raw
        assert not bool(torch.isnan(work).any())
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
