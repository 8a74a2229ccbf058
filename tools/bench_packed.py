#!/usr/bin/env python3
"""
The batch gather out of a series held as int16 codes (DLWP.model.PackedSeries -> dlwpcs_batch_gather_i16) against the gather out
of the same series held as fp32 (dlwpcs_batch_gather), both resident in HBM, in one process: one JSON line.

  * gather: microseconds per call of the two gathers a generator-fed training step makes -- the predictors (2 input time steps of
    every variable, bf16 out) and the targets (2 output time steps, fp32 out) -- at the production model's shape (C48, 7
    variables, batch 32) and at BASELINE config 5's (C96, 13 variables x 2 steps = 26 channels, batch 32).  Device events around
    --launches back-to-back launches captured as one graph, the two forms alternating, median of --reps windows after a warm-up
    window.  Every launch of a window has a sample list of its own, drawn over the whole record, and both the record (--rows) and
    what one window reads are larger than the 256 MB last-level cache, so the gathers read HBM as they do in training.  The
    output buffer is the same for every launch and both forms.  GB/s = (source bytes read + output bytes written) / time.
  * resident: bytes of both forms of the record timed here (measured from the objects) and of a 40-year record, 6-hourly and
    3-hourly (arithmetic): the packed form is half the fp32 form plus 8 bytes per variable.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'dlwp-cs_amd')]

import numpy as np   # noqa: E402
import torch         # noqa: E402

SHAPES = (('production_C48_7var', 48, 7), ('config5_C96_13var', 96, 13))
ITS = OTS = 2


def _windows(fns, launches, reps):
    """{name: median microseconds per call}: device events around `launches` launches fn(i) of each fn, alternating, reps windows"""
    # (a window is one captured graph of `launches` launches: the kernels take microseconds, less than the host needs to enqueue one)
    graphs = {}
    for name, fn in fns.items():
        fn(0)                                                   # loads the code object outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for i in range(launches):
                fn(i)                                           # launch i reads sample list i
        graphs[name] = g
    times = {k: [] for k in fns}
    for rep in range(reps + 1):
        for name, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            if rep:                                             # window 0 warms up
                times[name].append(1e3 * e0.elapsed_time(e1) / launches)
    return {k: float(np.median(v)) for k, v in times.items()}


def resident_bytes(T, V, N):
    fp32 = T * V * 6 * N * N * 4
    return {'rows': T, 'fp32_bytes': fp32, 'packed_bytes': fp32 // 2 + 8 * V}


def gather(a, dev):
    from DLWP import ops
    from DLWP.model import PackedSeries
    B, T = a.batch, a.rows
    out, res = {}, {}
    for name, N, V in SHAPES:
        S = 6 * N * N
        gen = torch.Generator(device=dev).manual_seed(N)
        arr = torch.empty((T, V, 6, N, N), dtype=torch.float32, device=dev)
        for t0 in range(0, T, 256):                             # (in slabs: the generator's temporaries stay small)
            arr[t0:t0 + 256].normal_(generator=gen)
        series = PackedSeries.pack(arr)
        assert series.device == arr.device and series.q.dtype == torch.int16
        res[name + '_timed_record'] = {'rows': T, 'fp32_bytes': arr.numel() * arr.element_size(), 'packed_bytes': series.nbytes}
        assert res[name + '_timed_record'] == resident_bytes(T, V, N)
        for rows, tag in ((58440, '40_years_6_hourly'), (116880, '40_years_3_hourly')):
            res['%s_%s' % (name, tag)] = resident_bytes(rows, V, N)
        var = torch.arange(V, dtype=torch.int32, device=dev)
        rng = np.random.default_rng(N)
        smp = torch.from_numpy(rng.integers(0, T - ITS - OTS, size=(a.launches, B)).astype(np.int32)).to(dev)
        p = torch.zeros((B, 6, N, N, ITS * V), dtype=torch.bfloat16, device=dev)
        t = torch.zeros((B, 6, N, N, OTS * V), dtype=torch.float32, device=dev)
        us = _windows({
            'predictors_fp32': lambda i: ops.batch_gather(arr, smp[i], var, p, ITS, 0, 1, 0, V, True),
            'predictors_packed': lambda i: ops.batch_gather(series, smp[i], var, p, ITS, 0, 1, 0, V, True),
            'targets_fp32': lambda i: ops.batch_gather(arr, smp[i], var, t, OTS, ITS, 1, 0, V, True),
            'targets_packed': lambda i: ops.batch_gather(series, smp[i], var, t, OTS, ITS, 1, 0, V, True),
        }, a.launches, a.reps)
        elems = B * ITS * V * S
        moved = {'predictors_fp32': elems * (4 + 2), 'predictors_packed': elems * (2 + 2),
                 'targets_fp32': elems * (4 + 4), 'targets_packed': elems * (2 + 4)}
        out[name] = {'batch': B, 'channels': ITS * V, 'elements': elems,
                     **{k + '_us': round(v, 2) for k, v in us.items()},
                     **{k + '_MB': round(moved[k] / 1e6, 2) for k in us},
                     **{k + '_GBs': round(moved[k] / v / 1e3, 1) for k, v in us.items()},
                     'predictors_packed_over_fp32': round(us['predictors_packed'] / us['predictors_fp32'], 3),
                     'targets_packed_over_fp32': round(us['targets_packed'] / us['targets_fp32'], 3)}
        del arr, series, p, t
        torch.cuda.empty_cache()
    return out, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=2920, help='rows of the record the gathers read (2920 = 2 years, 6-hourly)')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--reps', type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_packed: no HIP device (times are measured on the GPU or not at all)')
    from DLWP.keras import backend
    backend.set_device('cuda:0')
    times, res = gather(a, torch.device('cuda:0'))
    print(json.dumps({'resident': res, 'gather': times}))


if __name__ == '__main__':
    main()
