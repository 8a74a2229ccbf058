"""
Writes the offline-map fixtures of tests/test_remap.py with an independent netCDF writer (scipy.io.netcdf_file):
  g14_map_classic.nc  CDF-1 (version 1): synthetic map cubed sphere N=4 -> lat-lon 5 x 8, in the SCRIP / TempestRemap layout
  g14_map_64bit.nc    CDF-2 (version 2): the other direction, lat-lon 5 x 8 -> N=4, plus two record variables
  g14_remap.npz       the arrays written, under '<file tag>/<variable>'
The maps come from tests/remap_maps.py (sub-point sampling; not TempestRemap output).  Needs scipy; the test does not.
Run from the repository root: python tests/golden/gen_golden_remap.py
"""
import os
import sys

import numpy as np
from scipy.io import netcdf_file

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'dlwp-cs_amd')]
import remap_maps as rm                                   # noqa: E402


def write(path, version, a, records=None):
    f = netcdf_file(path, 'w', version=version)
    f.title = 'synthetic offline map (sub-point sampling), test fixture'
    n_s = a['row'].size
    if records:
        f.createDimension('rec', None)                     # the record (unlimited) dimension has to come first
        f.createDimension('three', 3)
    f.createDimension('n_a', a['n_a'])
    f.createDimension('n_b', a['n_b'])
    f.createDimension('n_s', n_s)
    f.createDimension('src_grid_rank', a['src_grid_dims'].size)
    f.createDimension('dst_grid_rank', a['dst_grid_dims'].size)
    out = {}
    for name, dim, dt in (('src_grid_dims', 'src_grid_rank', 'i4'), ('dst_grid_dims', 'dst_grid_rank', 'i4'),
                          ('yc_a', 'n_a', 'f8'), ('xc_a', 'n_a', 'f8'), ('yc_b', 'n_b', 'f8'), ('xc_b', 'n_b', 'f8'),
                          ('frac_b', 'n_b', 'f8'), ('row', 'n_s', 'i4'), ('col', 'n_s', 'i4'), ('S', 'n_s', 'f8')):
        val = np.ones(a['n_b']) if name == 'frac_b' else a[name]
        v = f.createVariable(name, dt, (dim,))
        v[:] = val
        if name.startswith(('yc', 'xc')):
            v.units = 'degrees'
        out[name] = np.asarray(val, dtype=dt)
    if records:
        for name, (dims, val) in records.items():
            v = f.createVariable(name, val.dtype.str[1:], dims)
            v[:] = val
            out[name] = val
    f.close()
    return out


def main():
    cube, ll = rm.Cube(4, rm.rotation(10., 5., 0.)), rm.LatLon(5, 8)
    fw = rm.map_arrays(cube, ll, s=2)
    bw = rm.map_arrays(ll, cube, s=2)
    rng = np.random.default_rng(14)
    recs = {'rec_a': (('rec', 'three'), rng.standard_normal((4, 3))), 'rec_b': (('rec',), np.arange(4, dtype=np.int32) * 7)}
    exp = {}
    for tag, v, a, r in (('classic', 1, fw, None), ('64bit', 2, bw, recs)):
        got = write(os.path.join(HERE, 'g14_map_%s.nc' % tag), v, a, r)
        for k, val in got.items():
            exp['%s/%s' % (tag, k)] = val
        exp['%s/n_a' % tag], exp['%s/n_b' % tag] = np.int64(a['n_a']), np.int64(a['n_b'])
    np.savez_compressed(os.path.join(HERE, 'g14_remap.npz'), **exp)


if __name__ == '__main__':
    main()
