#!/usr/bin/env python3
"""
Golden vectors for `mean_by_batch` / `std_by_batch` (reference DLWP/model/preprocessing.py:844-882): the two reference function
bodies, cut out of the reference file at generation time (the module itself imports netCDF4 and xarray, which are not installed
where this script runs, and neither function touches them) and executed on a stand-in for the DataArray they are handed:
`.shape`, `.dims`, `.size` and `.isel(**{dim: slice}).values`.  This script holds no reference program text.

Data: one float32 array of shape (37, 3, 6, 4, 4) -- 37 samples (a prime: every batch size leaves a ragged last batch), three
variables of different mean and spread treated as ONE array, as the two functions treat whatever they are given.
Recorded: the input, and per (axis in 0, 1) x (batch size in 1, 8, 100) the mean, the std computed from that mean, and the std
computed without one.  Output: tests/golden/g16_scaling.npz.  Tests read the .npz only.

Usage: DLWP_REFERENCE=<root of the reference checkout> python gen_golden_scaling.py     (CPU only)
"""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE = (37, 3, 6, 4, 4)
DIMS = ('sample', 'varlev', 'face', 'height', 'width')
BATCHES = (1, 8, 100)
AXES = (0, 1)


class DA(object):
    """the members of an xarray.DataArray the two functions read"""

    def __init__(self, values, dims):
        self.values, self.dims = values, tuple(dims)

    @property
    def shape(self):
        return self.values.shape

    @property
    def size(self):
        return self.values.size

    def isel(self, **indexers):
        idx = [slice(None)] * self.values.ndim
        for k, v in indexers.items():
            idx[self.dims.index(k)] = v
        return DA(self.values[tuple(idx)], self.dims)


def data():
    rng = np.random.default_rng(16)
    x = rng.standard_normal(SHAPE)
    x[:, 0] = x[:, 0] * 3. + 12.
    x[:, 1] = x[:, 1] * 0.5 - 2.
    x[:, 2] = x[:, 2] * 8. + 30. + 4. * np.sin(np.arange(SHAPE[0]) / 5.)[:, None, None, None]
    return x.astype(np.float32)


def main():
    ref = os.environ.get('DLWP_REFERENCE')
    if not ref:
        sys.exit(__doc__)
    src = open(os.path.join(ref, 'DLWP', 'model', 'preprocessing.py')).read()
    ns = {'np': np}
    for name in ('mean_by_batch', 'std_by_batch'):
        fn_src = re.search(r'^def %s\(.*?(?=^def |\Z)' % name, src, re.S | re.M).group(0)
        exec(compile(fn_src, 'preprocessing.py:' + name, 'exec'), ns)
    x = data()
    da = DA(x, DIMS)
    out = {'x': x, 'batches': np.asarray(BATCHES), 'axes': np.asarray(AXES)}
    for axis in AXES:
        for bs in BATCHES:
            key = 'axis%d_batch%d' % (axis, bs)
            mean = ns['mean_by_batch'](da, bs, axis)
            out['mean_' + key] = np.float64(mean)
            out['std_given_' + key] = np.float64(ns['std_by_batch'](da, bs, axis, mean=mean))
            out['std_' + key] = np.float64(ns['std_by_batch'](da, bs, axis))
    np.savez_compressed(os.path.join(HERE, 'g16_scaling.npz'), **out)
    for k in sorted(out):
        if k.startswith(('mean', 'std')):
            print(k, repr(float(out[k])))


if __name__ == '__main__':
    main()
