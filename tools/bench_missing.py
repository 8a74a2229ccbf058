#!/usr/bin/env python3
"""
Missing values on the device data path: what they cost.  One JSON line.

  * remap: `ops.sparse_map_apply(..., skipna=True)` (dlwpcs_sparse_map_apply_masked; with and without the fraction output)
    against the plain launch over the same data, with 20 % of the cells NaN and with none, for the conservative maps
    181 x 360 -> C48, C48 -> 181 x 360 and C48 -> 721 x 1440 over a (--fields, *grid) fp32 stack.  `masked_over_plain` is the
    ratio of the medians; the two kernels read the same bytes.
  * counts: `ops.missing_counts` over a (T, 7, 6, 48, 48) series of about --gb GB, fp32 and int16 codes, against the question
    it replaces -- `torch.isnan(x).any()` / `(q == -32768).any()` -- and against the device-to-device copy rate of the same
    array in the same run (`of_copy`: bytes read per second over the copy's bytes moved per second, as tools/bench_scaling.py
    reports it).
Device events around each call, median of --reps calls after one warm-up call.
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
    """median milliseconds of fn() over `reps` calls after one warm-up call"""
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


def _remap_case(m, axes, fields, reps, dev):
    from DLWP import ops
    gen = torch.Generator(device=dev).manual_seed(2)
    x = torch.randn((fields,) + tuple(m.src_shape), dtype=torch.float32, device=dev, generator=gen)
    holed = x.clone()
    holed[torch.rand(x.shape, device=dev, generator=gen) < 0.2] = float('nan')
    y = torch.empty((fields,) + tuple(m.dst_shape), dtype=torch.float32, device=dev)
    frac = torch.empty_like(y)
    plain = _time(lambda: ops.sparse_map_apply(m, x, axes, out=y), reps)
    out = {'entries': m.nnz, 'rows': m.n_b, 'fields': fields, 'plain_ms': round(plain, 4)}
    for tag, data in (('no_holes', x), ('holes_20pct', holed)):
        a = _time(lambda: ops.sparse_map_apply(m, data, axes, out=y, skipna=True), reps)
        b = _time(lambda: ops.sparse_map_apply(m, data, axes, out=y, skipna=True, frac_out=frac), reps)
        out[tag] = {'masked_ms': round(a, 4), 'masked_over_plain': round(a / plain, 3), 'with_frac_ms': round(b, 4),
                    'with_frac_over_plain': round(b / plain, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gb', type=float, default=1.0, help='size of the fp32 series of the count pass')
    ap.add_argument('--fields', type=int, default=28, help='fields per remap call (4 times x 7 variables)')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--skip-quarter-degree', action='store_true', help='leave out C48 -> 721 x 1440 (its map takes the longest to make)')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_missing: no HIP device (times are measured on the GPU or not at all)')
    from DLWP import ops
    from DLWP.remap import CubeSphereGrid, LatLonGrid, conservative_maps
    dev = torch.device('cuda:0')
    out = {'reps': a.reps, 'device': torch.cuda.get_device_name(0)}

    # ---- masked against plain application ----
    cube = CubeSphereGrid(48)
    fwd, inv = conservative_maps(cube, LatLonGrid.cells(181, 360), device=dev)
    remap = {'ll181x360_to_c48': _remap_case(fwd, (1, 2), a.fields, a.reps, dev),
             'c48_to_ll181x360': _remap_case(inv, (1, 2, 3), a.fields, a.reps, dev)}
    if not a.skip_quarter_degree:
        _, inv_q = conservative_maps(cube, LatLonGrid.cells(721, 1440), device=dev)
        remap['c48_to_ll721x1440'] = _remap_case(inv_q, (1, 2, 3), a.fields, a.reps, dev)
        del inv_q
    out['remap'] = remap
    torch.cuda.empty_cache()

    # ---- the count pass ----
    V, S = 7, 6 * 48 * 48
    T = max(int(a.gb * 1e9 / (V * S * 4)), 1)
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((T, V, 6, 48, 48), dtype=torch.float32, device=dev, generator=gen)
    x[T // 2, 3, 2, 5, 5] = float('nan')
    y = torch.empty_like(x)
    counts = {'shape': [T, V, 6, 48, 48]}
    for tag, data, twin, question in (('fp32', x, y, lambda t: torch.isnan(t).any()),
                                      ('int16', None, None, lambda t: (t == -32768).any())):
        if data is None:
            data = (x * 1000).clamp(-32767, 32767).to(torch.int16)
            data[T // 2, 3, 2, 5, 5] = -32768
            del x, y
            torch.cuda.empty_cache()
            twin = torch.empty_like(data)
        nbytes = data.numel() * data.element_size()
        copy_ms = _time(lambda: twin.copy_(data), a.reps)
        copy_gbs = 2 * nbytes / copy_ms / 1e6
        ours = _time(lambda: ops.missing_counts(data), a.reps)
        theirs = _time(lambda: question(data), a.reps)
        assert int(ops.missing_counts(data).sum().item()) == 1
        gbs = nbytes / ours / 1e6
        counts[tag] = {'MB': round(nbytes / 1e6, 1), 'copy_ms': round(copy_ms, 3), 'copy_GBs': round(copy_gbs, 1),
                       'count_ms': round(ours, 3), 'GBs': round(gbs, 1), 'of_copy': round(gbs / copy_gbs, 3),
                       'torch_any_ms': round(theirs, 3), 'torch_over_ours': round(theirs / ours, 2)}
    out['counts'] = counts
    print(json.dumps(out))


if __name__ == '__main__':
    main()
