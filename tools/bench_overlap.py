"""
Time conservative map generation on the device (dlwpcs_overlap_count / dlwpcs_overlap_fill, csrc/overlap.hip) for two
production-sized grid pairs:
  M1  181 x 360 lat-lon cells with centres on the poles -> C48
  M2  721 x 1440 (the ERA5 quarter-degree grid, descending latitudes) -> C96
Prints ONE JSON line: per pair the device time of the two launches (device events, mean of --iters calls after --warmup; the
scan and the read-back of the entry count between them are included in `total_us`), the entry count, the worst residual of
each marginal (row sums against the lat-lon cell areas, column sums against the cube cell areas), and for M1 the host twin's
time for the same matrix.

python tools/bench_overlap.py [--iters 5] [--warmup 1] [--no-host]
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
from DLWP.remap import CubeSphereGrid, LatLonGrid, overlap_areas      # noqa: E402
from DLWP.remap.overlap import DUST                       # noqa: E402


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


def run(name, cube, ll, args, host):
    dev = torch.device('cuda:0')
    row_ptr, col, area = ops.overlap_csr(cube, ll, DUST, dev)
    total = _events(lambda: ops.overlap_csr(cube, ll, DUST, dev), args.warmup, args.iters)
    # the two launches alone, on buffers that exist
    d = nat.OverlapDesc()
    d.N, d.n_lat, d.n_lon, d.dust = cube.N, ll.n_lat, ll.n_lon, DUST
    fr = np.ascontiguousarray(cube.frames)
    ctypes.memmove(ctypes.addressof(d.frames), fr.ctypes.data, fr.nbytes)
    sl, lo = torch.from_numpy(ll.sin_lat_edges.copy()).to(dev), torch.from_numpy(ll.lon_edges_rad.copy()).to(dev)
    counts = torch.empty(ll.n_cells, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    lib = nat.lib()
    count = _events(lambda: nat.check(lib.dlwpcs_overlap_count(ctypes.byref(d), sl.data_ptr(), lo.data_ptr(), counts.data_ptr(), s),
                                      'count'), args.warmup, args.iters)
    fill = _events(lambda: nat.check(lib.dlwpcs_overlap_fill(ctypes.byref(d), sl.data_ptr(), lo.data_ptr(), row_ptr.data_ptr(),
                                                             col.data_ptr(), area.data_ptr(), area.numel(), s), 'fill'),
                   args.warmup, args.iters)
    rp, c, A = row_ptr.cpu().numpy(), col.cpu().numpy(), area.cpu().numpy()
    r = np.repeat(np.arange(ll.n_cells), np.diff(rp))
    res_ll = float(np.abs(np.bincount(r, A, ll.n_cells) / ll.area.ravel() - 1.).max())
    res_cs = float(np.abs(np.bincount(c, A, cube.n_cells) / cube.area.ravel() - 1.).max())
    out = {'case': name, 'entries': int(A.size), 'count_us': round(count, 1), 'fill_us': round(fill, 1), 'total_us': round(total, 1),
           'residual_latlon': float('%.3g' % res_ll), 'residual_cube': float('%.3g' % res_cs)}
    if host:
        t = time.perf_counter()
        h = overlap_areas(cube, ll)
        out['host_us'] = round((time.perf_counter() - t) * 1e6, 0)
        out['host_same_pattern'] = bool(np.array_equal(h[0], rp) and np.array_equal(h[1], c))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--no-host', action='store_true')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    res = [run('M1 181x360 (pole-centred) -> C48', CubeSphereGrid(48),
               LatLonGrid.from_centres(np.linspace(-90., 90., 181), np.arange(360.)), args, not args.no_host),
           run('M2 721x1440 -> C96', CubeSphereGrid(96),
               LatLonGrid.from_centres(np.linspace(90., -90., 721), np.arange(1440) * 0.25), args, False)]
    print(json.dumps({'map_generation': res}), flush=True)


if __name__ == '__main__':
    main()
