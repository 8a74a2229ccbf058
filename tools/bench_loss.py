#!/usr/bin/env python3
"""
ms / training step of BASELINE config 3 (unet2 C48, 14 channels, B = 32; bf16 and fp32) under each training loss the engine
runs: 'mse', latitude-weighted MSE (the CS per-cell latitude field), keras 'mae' and the latitude-weighted anomaly-correlation
loss with a climatology (reference Azure/train_tf.py:346-357).  One process, one model per loss, the losses timed in
interleaved rounds (A/B/A/B) so that clock drift hits all alike; each timing is K captured-graph steps between two events.

    python tools/bench_loss.py [--steps 50] [--warmup 10] [--rounds 2] [--dtypes bf16,f32]

Prints one JSON line per dtype: {"dtype", "ms_per_step": {loss: [round values]}, "median": {loss: ms}}.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'dlwp-cs_amd'))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402


def _losses(N, C):
    from DLWP import custom
    from DLWP.keras import losses
    rng = np.random.default_rng(1)
    lats = rng.uniform(-89.0, 89.0, (6, N, N))
    clim = (0.3 * rng.standard_normal((1, 6, N, N, C))).astype(np.float32)
    shape = (6, N, N, C)
    return {'mse': 'mse',
            'lat_mse': custom.latitude_weighted_loss(losses.mse, lats, shape, weighting='midlatitude'),
            'mae': losses.mae,
            'lat_acc': custom.latitude_weighted_loss(custom.anomaly_correlation_loss(clim, regularize_mean='mse'), lats,
                                                     shape, weighting='midlatitude')}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--dtypes', default='bf16,f32')
    a = ap.parse_args()
    from DLWP.keras import Input, Model, backend
    from DLWP.model.cs_unet import CubeSphereNet
    backend.set_device('cuda:0')
    N, C, B = 48, 14, 32
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    x = torch.tensor(rng.standard_normal((B, 6, N, N, C)).astype(np.float32), device=dev)
    t = torch.tensor(rng.standard_normal((B, 6, N, N, C)).astype(np.float32), device=dev)
    for dt in a.dtypes.split(','):
        dtype = 'bfloat16' if dt == 'bf16' else 'float32'
        models = {}
        for name, loss in _losses(N, C).items():
            backend.set_compute_dtype(dtype)
            try:
                np.random.seed(3)
                net = CubeSphereNet(base_filter_number=32, output_channels=C)
                inp = Input(shape=(6, N, N, C), name='main_input')
                model = Model(inputs=inp, outputs=net.unet2(inp))
            finally:
                backend.set_compute_dtype('float32')
            model.compile(optimizer='adam', loss=loss)
            dx = [x.to(torch.bfloat16) if dtype == 'bfloat16' else x]
            for _ in range(a.warmup):
                model.train_on_device_batch(dx, [t])
            torch.cuda.synchronize()
            models[name] = (model, dx)
        res = {k: [] for k in models}
        for _ in range(a.rounds):
            for name, (model, dx) in models.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    model.train_on_device_batch(dx, [t])
                e1.record()
                e1.synchronize()
                res[name].append(round(e0.elapsed_time(e1) / a.steps, 4))
        print(json.dumps({'dtype': dt, 'B': B, 'steps': a.steps, 'ms_per_step': res,
                          'median': {k: float(np.median(v)) for k, v in res.items()}}), flush=True)
        del models


if __name__ == '__main__':
    main()
