"""
Time the bilinear sampling map (dlwpcs_cube_bilinear, csrc/bilinear.hip) at two production sizes:
  S1  the centres of 181 x 360 (rows on the poles) sampled from C48
  S2  the centres of 721 x 1440 (the ERA5 quarter-degree grid, descending latitudes) sampled from C96
Prints ONE JSON line.  Per size: the device time of the one launch on points that lie on the device (`kernel_us`) and of
point_weights(device=...) on the same tensors, which adds the range check and its read-back (`point_weights_us`; device events,
mean of --iters calls after --warmup), the wall clock of bilinear_map(device=...) as a user calls it (upload, launch,
read-back and the OfflineMap's construction on the host), the host twin's wall clock for the same weights, the share of
points both give to the same dual face and the largest difference of their weights there; then sample_array of a
(40, 4, 6, N, N) fp32 forecast through the bilinear map and inverse_remap_array of the same forecast through the first-order
conservative map of the same grids (device events), with the entries of both maps.

python tools/bench_bilinear.py [--iters 10] [--warmup 2] [--no-host]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'dlwp-cs_amd')]
from DLWP import _native as nat                           # noqa: E402
from DLWP import ops                                      # noqa: E402
from DLWP.remap.bilinear import cube_edges                # noqa: E402
from DLWP.remap import CubeSphereGrid, CubeSphereRemap, LatLonGrid, bilinear_map, point_weights      # noqa: E402


def _events(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def _wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e6


def run(name, cube, ll, args, host):
    dev = torch.device('cuda:0')
    yc, xc = (g.ravel() for g in np.meshgrid(ll.lat, ll.lon, indexing='ij'))
    la, lo = torch.from_numpy(yc.copy()).to(dev), torch.from_numpy(xc.copy()).to(dev)
    col, w = ops.cube_bilinear(cube, la, lo, dev)
    weights = _events(lambda: ops.cube_bilinear(cube, la, lo, dev), args.warmup, args.iters)
    # the launch alone, on buffers that exist
    d = nat.CubeBilinearDesc()
    d.N, d.n_points = cube.N, yc.size
    fr, ed = np.ascontiguousarray(cube.frames), np.ascontiguousarray(cube_edges())
    ctypes.memmove(ctypes.addressof(d.frames), fr.ctypes.data, fr.nbytes)
    ctypes.memmove(ctypes.addressof(d.edge), ed.ctypes.data, ed.nbytes)
    s = torch.cuda.current_stream().cuda_stream
    lib = nat.lib()
    kernel = _events(lambda: nat.check(lib.dlwpcs_cube_bilinear(ctypes.byref(d), la.data_ptr(), lo.data_ptr(), col.data_ptr(),
                                                                w.data_ptr(), s), 'cube_bilinear'), args.warmup, args.iters)
    m, map_us = _wall(lambda: bilinear_map(cube, latlon=ll, device=dev))
    out = {'case': name, 'points': int(yc.size), 'kernel_us': round(kernel, 1), 'point_weights_us': round(weights, 1),
           'bilinear_map_us': round(map_us, 0)}
    if host:
        (h_col, h_w), host_us = _wall(lambda: point_weights(cube, yc, xc))
        same = (h_col == col.cpu().numpy()).all(axis=1)
        out.update(host_us=round(host_us, 0), host_same_cells=float('%.6f' % same.mean()),
                   host_max_diff=float('%.3g' % np.abs(h_w - w.cpu().numpy())[same].max()))
    # applying the map: bilinear against first-order conservative, the same grids and forecast
    r = CubeSphereRemap(verbose=False)
    _, inv = r.generate_maps(grid=cube, latlon=ll, device=dev)
    r.sampling_map = m
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((40, 4) + cube.shape, generator=g, device=dev)
    out['sample_array_us'] = round(_events(lambda: r.sample_array(x), args.warmup, args.iters), 1)
    out['inverse_remap_array_us'] = round(_events(lambda: r.inverse_remap_array(x), args.warmup, args.iters), 1)
    out['entries_bilinear'], out['entries_conservative'] = int(m.nnz), int(inv.nnz)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-host', action='store_true')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    res = [run('S1 C48 -> 181x360 centres', CubeSphereGrid(48),
               LatLonGrid.from_centres(np.linspace(-90., 90., 181), np.arange(360.)), args, not args.no_host),
           run('S2 C96 -> 721x1440 centres', CubeSphereGrid(96),
               LatLonGrid.from_centres(np.linspace(90., -90., 721), np.arange(1440) * 0.25), args, not args.no_host)]
    print(json.dumps({'bilinear_sampling': res}), flush=True)


if __name__ == '__main__':
    main()
