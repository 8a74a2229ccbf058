#!/usr/bin/env python3
"""
Golden vectors for the forecast scores `forecast_error`, `persistence_error` and `climo_error` (reference DLWP/verify.py:18-164):
the reference function bodies, cut out of the reference file at generation time (as gen_golden_verify.py does), executed on numpy
inputs.  Weighted cases hand the functions an ndarray subclass carrying `.lat` in a numpy-broadcastable layout.
Cases: mse / mae / rmse / acc x aligned / lagged x weighted or not x axis None / int / tuple x with and without NaNs (including an
all-NaN slice) x climatology of spatial, (1, ...) and (T, ...) shape; persistence and climatology cases; lagged and persistence
cases whose forecast / predictors have more times than the verification series.
Output: tests/golden/g13_scores.npz (inputs, one result per case, the case table as JSON).  Runs ONLY in the build container.
"""
import json
import os
import re
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
F, T, S = 3, 6, (2, 3, 4)


class WithLat(np.ndarray):
    """ndarray + a `.lat` attribute (what `weighted=True` reads)"""
    def __new__(cls, a, lat):
        o = np.asarray(a).view(cls)
        o.lat = lat
        return o

    def __array_finalize__(self, obj):
        self.lat = getattr(obj, 'lat', None)


class _XR(object):
    class DataArray(object):
        pass


def _fns():
    src = open(os.path.join(REF, 'DLWP', 'verify.py')).read()
    ns = {'np': np, 'xr': _XR, 'warnings': warnings}
    for name in ('forecast_error', 'persistence_error', 'climo_error'):
        fn_src = re.search(r'^def %s\(.*?(?=^def |\Z)' % name, src, re.S | re.M).group(0)
        exec(compile(fn_src, 'verify.py:' + name, 'exec'), ns)
    return ns['forecast_error'], ns['persistence_error'], ns['climo_error']


def inputs():
    rng = np.random.default_rng(13)
    d = {
        'forecast': rng.standard_normal((F, T) + S).astype(np.float32),
        'valid_f': rng.standard_normal((F, T) + S).astype(np.float32),
        'valid_s': rng.standard_normal((T,) + S).astype(np.float32),
        'clim_sp': (0.3 * rng.standard_normal(S)).astype(np.float32),
        'clim_1': (0.3 * rng.standard_normal((1,) + S)).astype(np.float32),
        'clim_t': (0.3 * rng.standard_normal((T,) + S)).astype(np.float32),
        'lat': rng.uniform(-80., 80., S[1:]).astype(np.float64),
        'predictors': rng.standard_normal((T,) + S).astype(np.float32),
    }
    # a forecast with more initialisation times than the series (the lagged form reads forecast[f, :V - f])
    d['forecast_long'] = rng.standard_normal((F, T + 2) + S).astype(np.float32)
    d['predictors_long'] = rng.standard_normal((T + 3,) + S).astype(np.float32)
    for k in ('forecast', 'valid_f', 'valid_s', 'predictors'):
        x = d[k + '_nan'] = d[k].copy()
        m = rng.random(x.shape) < 0.15
        x[m] = np.nan
        x[..., 0, 0, 0] = np.nan                         # an all-NaN slice when the spatial axes are kept
    return d


def cases():
    out = []
    for method in ('mse', 'mae', 'rmse', 'acc'):
        for weighted in (False, True):
            for nan in (False, True):
                for axis in (None, 1, (1, 2), (2, 3, 4), -1):
                    clims = ('clim_sp', 'clim_1', 'clim_t', None) if method == 'acc' else (None,)
                    for clim in clims:
                        out.append(dict(fn='forecast_error', form='aligned', method=method, weighted=weighted, nan=nan,
                                        axis=axis, clim=clim))
                for axis in (None, 0, (0, 2)):
                    for clim in ('clim_sp', 'clim_1'):
                        if clim == 'clim_1' and method != 'acc' and axis is not None:
                            continue
                        out.append(dict(fn='forecast_error', form='lagged', method=method, weighted=weighted, nan=nan,
                                        axis=axis, clim=clim))
    for method in ('mse', 'mae', 'rmse'):
        for weighted in (False, True):
            for axis in (None, 0, (0, 2)):
                out.append(dict(fn='forecast_error', form='lagged', method=method, weighted=weighted, nan=False, axis=axis,
                                clim='clim_sp', long=True))
                out.append(dict(fn='persistence_error', method=method, weighted=weighted, nan=False, axis=axis, long=True))
    for fn in ('persistence_error', 'climo_error'):
        for method in ('mse', 'mae', 'rmse'):
            for weighted in (False, True):
                for nan in (False, True):
                    for axis in (None, 0, (0, 1)):
                        out.append(dict(fn=fn, method=method, weighted=weighted, nan=nan, axis=axis))
    return out


def case_key(i, c):
    return 'case%03d' % i


def run_case(fns, d, c, host=None):
    """evaluate case c with `fns` = (forecast_error, persistence_error, climo_error) on the inputs d"""
    fe, pe, ce = fns
    sfx = '_nan' if c['nan'] else ''
    axis = tuple(c['axis']) if isinstance(c['axis'], list) else c['axis']
    wrap = (lambda a: WithLat(a, d['lat'])) if c['weighted'] else (lambda a: a)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if c['fn'] == 'forecast_error':
            valid = wrap(d['valid_f' + sfx] if c['form'] == 'aligned' else d['valid_s' + sfx])
            clim = None if c['clim'] is None else d[c['clim']]
            return fe(d['forecast_long' if c.get('long') else 'forecast' + sfx], valid, method=c['method'], axis=axis, weighted=c['weighted'], climatology=clim)
        if c['fn'] == 'persistence_error':
            return pe(d['predictors_long' if c.get('long') else 'predictors' + sfx], wrap(d['valid_s' + sfx]), F, method=c['method'], axis=axis,
                      weighted=c['weighted'])
        return ce(wrap(d['valid_s' + sfx]), F, method=c['method'], axis=axis, weighted=c['weighted'])


def main():
    fns = _fns()
    d = inputs()
    out = dict(d)
    table = cases()
    for i, c in enumerate(table):
        r = np.asarray(run_case(fns, d, c), dtype=np.float64)
        out[case_key(i, c)] = r
    out['cases'] = np.array(json.dumps(table))
    np.savez_compressed(os.path.join(HERE, 'g13_scores.npz'), **out)
    print('wrote %d cases' % len(table))


if __name__ == '__main__':
    main()
