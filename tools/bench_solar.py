#!/usr/bin/env python3
"""
Solar forcing computed on the device (DLWP.util.SolarForcing -> dlwpcs_solar_fill) against the dense array it replaces
(dlwpcs_batch_gather out of a (T, 1, 6, N, N) fp32 array resident in HBM): one JSON line.

  * kernels: microseconds per call of `solar_fill` and of the `batch_gather` it replaces, at the production model's shapes
    (batch 32, 2 input time steps, 4 variables + the solar channel; C48 and C96; fp32 and bf16 output), for the two calls a
    step makes: the solar channel of the main input (channels interleaved with the variables: Ctot = 10, c_off = 4, c_stride = 5)
    and a solar input of a later integration step (64 one-channel rows).  Device events around --launches back-to-back launches,
    the two forms alternating, median of --reps windows after a warm-up window.  Every launch of a window has a sample list of its
    own, drawn over the whole record, and the record (--rows, 10 years: 0.8 GB at C48, 3.2 GB at C96) is larger than the 256 MB
    last-level cache, as is what one window reads (--launches x 64 rows: 0.7 GB / 2.8 GB): the gather reads mostly HBM, as it does
    in training.  The output buffer is the same for every launch (7-71 MB), for both forms.  GB/s = output bytes written / time
    (the gather also reads 4 B per element).
  * resident: bytes each form keeps in HBM for the record timed here and for a 40-year 6-hourly record (58 440 rows), from shapes.
  * rollout: milliseconds per forecast of `Model.rollout_with_forcing` for the production wiring (unet2, base 32, integration_steps 2,
    solar + constants inputs, C48; --sequence-steps applications, --batch samples) fed the dense array of --rollout-rows rows and fed
    the SolarForcing: replayed graphs (the dense form copies the whole array into the graph's buffer per call), host clock around
    a call that ends in a device synchronise, median of --reps after warm-up calls, the two forms alternating.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'dlwp-cs_amd')]

import numpy as np   # noqa: E402
import torch         # noqa: E402


def cube_latlon(N):
    """cell centres (degrees) of an equiangular cubed sphere, (6, N, N) each"""
    a = -np.pi / 4 + (np.arange(N) + 0.5) * np.pi / (2 * N)
    ta, tb = np.meshgrid(np.tan(a), np.tan(a))                  # width, height
    one = np.ones_like(ta)
    faces = [(one, ta, tb), (-ta, one, tb), (-one, -ta, tb), (ta, -one, tb), (-tb, ta, one), (tb, ta, -one)]
    p = np.array([np.stack(f, axis=-1) for f in faces])
    p /= np.linalg.norm(p, axis=-1, keepdims=True)
    return np.rad2deg(np.arcsin(p[..., 2])), np.mod(np.rad2deg(np.arctan2(p[..., 1], p[..., 0])), 360.)


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


def kernels(a, dev):
    from DLWP import ops
    from DLWP.util import SolarForcing
    B, its, V = a.batch_kernel, 2, 4
    T = a.rows
    dates = np.datetime64('1990-01-01T00', 'ns') + np.arange(T) * np.timedelta64(6, 'h')
    out = {}
    for N in (48, 96):
        lat, lon = cube_latlon(N)
        sf = SolarForcing(dates, lat, lon)
        row, cell = sf.tables(dev)
        dense = sf.to_device(dev).unsqueeze(1)                  # (T, 1, 6, N, N)
        S = 6 * N * N
        zero = torch.zeros(1, dtype=torch.int32, device=dev)
        rng = np.random.default_rng(N)
        smp = torch.from_numpy(rng.integers(0, T - its, size=(a.launches, B)).astype(np.int32)).to(dev)
        smp2 = torch.from_numpy(rng.integers(0, T, size=(a.launches, B * its)).astype(np.int32)).to(dev)
        for dt, name in ((torch.float32, 'fp32'), (torch.bfloat16, 'bf16')):
            main = torch.zeros((B, 6, N, N, its * (V + 1)), dtype=dt, device=dev)
            sol = torch.zeros((B * its, 6, N, N, 1), dtype=dt, device=dev)
            us = _windows({
                'main_fill': lambda i: ops.solar_fill(row, cell, smp[i], main, its, 0, 1, V, V + 1, True),
                'main_gather': lambda i: ops.batch_gather(dense, smp[i], zero, main, its, 0, 1, V, V + 1, True),
                'solar_fill': lambda i: ops.solar_fill(row, cell, smp2[i], sol, 1, 0, 1, 0, 1, True),
                'solar_gather': lambda i: ops.batch_gather(dense, smp2[i], zero, sol, 1, 0, 1, 0, 1, True),
            }, a.launches, a.reps)
            nbytes = B * its * S * main.element_size()
            out['C%d_%s' % (N, name)] = {
                'out_MB': round(nbytes / 1e6, 3),
                **{k + '_us': round(v, 2) for k, v in us.items()},
                **{k + '_GBs': round(nbytes / v / 1e3, 1) for k, v in us.items()},
            }
        del dense, sf
        torch.cuda.empty_cache()
    return out


def resident(a):
    out = {}
    for N in (48, 96):
        S = 6 * N * N
        for T, name in ((a.rows, 'timed_record'), (58440, '40_years_6_hourly')):
            out['C%d_%s' % (N, name)] = {'rows': T, 'dense_bytes': T * S * 4, 'tables_bytes': (T * 4 + S * 3) * 8}
    return out


def rollout(a, dev):
    from DLWP.keras import backend
    from DLWP.model import DLWPFunctional
    from DLWP.model.cs_unet import build_cs_model
    from DLWP.model.generators import ArrayDataGenerator
    from DLWP.util import SolarForcing
    N, V, K, its, n_out, B = 48, 4, 2, 2, 2, a.batch
    T = a.rollout_rows
    dates = np.datetime64('1990-01-01T00', 'ns') + np.arange(T) * np.timedelta64(6, 'h')
    lat, lon = cube_latlon(N)
    sf = SolarForcing(dates, lat, lon)
    dense = sf.to_device(dev)                                   # (T, 6, N, N): a device tensor takes the dense path as it is
    rng = np.random.default_rng(1)
    Td = 64                                                     # the data rows the initial states come from
    arr = rng.standard_normal((Td, V, 6, N, N)).astype(np.float32)
    const = rng.standard_normal((K, 6, N, N)).astype(np.float32)
    out = {'rows': T, 'batch': B, 'sequence_steps': a.sequence_steps, 'dense_MB': round(dense.numel() * 4 / 1e6, 1)}
    samples = np.arange(B, dtype=np.int64) * 3
    for dtype in ('float32', 'bfloat16'):
        dlwp = DLWPFunctional(is_convolutional=True, time_dim=its)
        gen = ArrayDataGenerator(dlwp, arr, rank=3, batch_size=B, input_time_steps=its, output_time_steps=its, sequence=n_out,
                                 insolation_array=sf, constants=const, channels_last=True, device=dev, dtype=dtype)
        backend.set_compute_dtype(dtype)
        try:
            np.random.seed(3)
            model = build_cs_model(gen.convolution_shape, its * V, 'unet2', base_filter_number=32, integration_steps=n_out,
                                   io_time_steps=its, insolation_shape=gen.insolation_shape, constants_shape=(6, N, N, K))
        finally:
            backend.set_compute_dtype('float32')
        dlwp.build_model(model, loss='mse', optimizer='adam')
        p, _ = gen.generate(samples)

        def call(ins):
            model.rollout_with_forcing(p, a.sequence_steps, insolation=ins, start_index=samples, io_time_steps=its)
            torch.cuda.synchronize()
        forms = {'dense': dense, 'solar_forcing': sf}
        for _ in range(3):                                      # eager, capture, replay
            for ins in forms.values():
                call(ins)
        ts = {k: [] for k in forms}
        for _ in range(a.reps):
            for k, ins in forms.items():
                t0 = time.perf_counter()
                call(ins)
                ts[k].append(time.perf_counter() - t0)
        replayed = sum(1 for k, g in model._infer_graphs.items() if k[0] == 'forcing' and g)
        out[dtype] = {**{k + '_ms': round(1e3 * float(np.median(v)), 3) for k, v in ts.items()}, 'graphs_replayed': replayed}
        model.release_rollout_buffers()
        del model, dlwp, gen
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=14600, help='rows of the record the kernels read (14600 = 10 years, 6-hourly)')
    ap.add_argument('--rollout-rows', type=int, default=14600, help='rows of the dense array the rollout is fed (10 years)')
    ap.add_argument('--batch-kernel', type=int, default=32)
    ap.add_argument('--batch', type=int, default=2, help='samples per forecast')
    ap.add_argument('--sequence-steps', type=int, default=10, help='model applications per forecast (10 = 40 time steps)')
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--no-rollout', action='store_true')
    a = ap.parse_args()
    out = {'resident': resident(a)}
    if not torch.cuda.is_available():
        raise SystemExit('bench_solar: no HIP device (times are measured on the GPU or not at all)')
    from DLWP.keras import backend
    backend.set_device('cuda:0')
    dev = torch.device('cuda:0')
    out['kernels'] = kernels(a, dev)
    if not a.no_rollout:
        out['rollout_C48'] = rollout(a, dev)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
