#!/usr/bin/env python3
"""
Golden vectors for the training losses of the reference (/root/reference/DLWP/custom.py:1543-1676): the bodies of
`latitude_weighted_loss`, `anomaly_correlation` and `anomaly_correlation_loss`, cut out of the reference file at generation
time, executed under a numpy stand-in for the keras backend `K` and for keras' `mean_squared_error` / `mean_absolute_error`
(mean over the last axis).  Keras' loss reduction -- the mean of the returned tensor -- is applied explicitly.  Stored per
case: the weight field (latitude-weighted cases) and the reduced loss value.  Output: tests/golden/g12_losses.npz.
Runs ONLY in the build container.
"""
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'


class _Var(np.ndarray):
    """K.zeros(...) / K.variable(...): an fp32 array with .assign"""
    def assign(self, v):
        self[...] = v


class K(object):
    @staticmethod
    def zeros(shape):
        return np.zeros(shape, dtype=np.float32).view(_Var)

    @staticmethod
    def ones(shape):
        return np.ones(shape, dtype=np.float32)

    @staticmethod
    def variable(value, name=None):
        return np.array(value, dtype=np.float32).view(_Var)

    @staticmethod
    def cast_to_floatx(x):
        return np.asarray(x, dtype=np.float32)

    cos = staticmethod(np.cos)
    sin = staticmethod(np.sin)
    sqrt = staticmethod(np.sqrt)
    square = staticmethod(np.square)
    abs = staticmethod(np.abs)

    @staticmethod
    def pow(x, a):
        return np.power(x, a)

    @staticmethod
    def expand_dims(x, axis=-1):
        return np.expand_dims(x, axis)

    @staticmethod
    def repeat_elements(x, rep, axis):
        return np.repeat(x, rep, axis=axis)

    @staticmethod
    def mean(x, axis=None):
        return np.mean(x, axis=tuple(axis) if isinstance(axis, list) else axis)


def mean_squared_error(y_true, y_pred):
    return np.mean(np.square(y_pred - y_true), axis=-1)


def mean_absolute_error(y_true, y_pred):
    return np.mean(np.abs(y_pred - y_true), axis=-1)


def keras_value(loss_fn, y_true, y_pred):
    """keras' reduction of the loss function's tensor (SUM_OVER_BATCH_SIZE without sample weights: the mean)"""
    return float(np.mean(np.asarray(loss_fn(y_true, y_pred))))


def main():
    src = open(os.path.join(REF, 'DLWP', 'custom.py')).read()
    ns = {'np': np, 'K': K, 'mean_squared_error': mean_squared_error, 'mean_absolute_error': mean_absolute_error}
    for name in ('latitude_weighted_loss', 'anomaly_correlation', 'anomaly_correlation_loss'):
        fn_src = re.search(r'^def %s\(.*?(?=^def |^# Compatibility|\Z)' % name, src, re.S | re.M).group(0)
        exec(compile(fn_src, 'custom.py:%s' % name, 'exec'), ns)
    lwl, ac, acl = ns['latitude_weighted_loss'], ns['anomaly_correlation'], ns['anomaly_correlation_loss']

    rng = np.random.default_rng(12)
    B, N, C = 2, 4, 3
    lats = rng.uniform(-89.0, 89.0, (6, N, N))
    y_true = (rng.standard_normal((B, 6, N, N, C)) + 0.5).astype(np.float32)
    y_pred = (y_true + 0.7 * rng.standard_normal((B, 6, N, N, C))).astype(np.float32)
    clim = (0.3 * rng.standard_normal((1, 6, N, N, C)) + 0.2).astype(np.float32)
    y_true_cf = np.ascontiguousarray(np.moveaxis(y_true, -1, 1))
    y_pred_cf = np.ascontiguousarray(np.moveaxis(y_pred, -1, 1))
    out = {'lats': lats, 'y_true': y_true, 'y_pred': y_pred, 'clim': clim, 'y_true_cf': y_true_cf, 'y_pred_cf': y_pred_cf}
    names = []

    def put(key, fn, cf=False, weights=True):
        names.append(key)
        yt, yp = (y_true_cf, y_pred_cf) if cf else (y_true, y_pred)
        out[key + '_loss'] = np.float64(keras_value(fn, yt, yp))
        if weights:
            free = dict(zip(fn.__code__.co_freevars, (c.cell_contents for c in fn.__closure__)))
            out[key + '_w'] = np.asarray(free['weights'], dtype=np.float32)      # lat_loss's weight field

    # latitude-weighted mse / mae: CS channels_last at axis=-2, both weightings; channels_first at axis=-1; lats=None
    for wt in ('cosine', 'midlatitude'):
        put('lat_mse_cl_%s' % wt, lwl(mean_squared_error, lats, (6, N, N, C), axis=-2, weighting=wt))
        put('lat_mae_cl_%s' % wt, lwl(mean_absolute_error, lats, (6, N, N, C), axis=-2, weighting=wt))
        put('lat_mse_cf_%s' % wt, lwl(mean_squared_error, lats, (C, 6, N, N), axis=-1, weighting=wt), cf=True)
    put('lat_mse_none', lwl(mean_squared_error, None, (6, N, N, C)))
    # anomaly correlation: with / without a climatology, every built regulariser, reverse both ways
    for reg in (None, 'mse', 'mae', 'global'):
        for rev in (True, False):
            for m in (None, clim):
                key = 'acc_%s_%s_%s' % (reg, 'rev' if rev else 'fwd', 'clim' if m is not None else 'zero')
                put(key, acl(m, regularize_mean=reg, reverse=rev), weights=False)
            key = 'acfn_%s_%s' % (reg, 'rev' if rev else 'fwd')
            put(key, lambda t, p, reg=reg, rev=rev: ac(t, p, regularize_mean=reg, reverse=rev), weights=False)
    # latitude-weighted anomaly correlation (reference Azure/train_tf.py:346-357)
    for reg in ('mse', None):
        put('lat_acc_%s' % reg, lwl(acl(clim, regularize_mean=reg), lats, (6, N, N, C), axis=-2, weighting='midlatitude'))
    out['cases'] = np.array(names)
    np.savez(os.path.join(HERE, 'g12_losses.npz'), **out)
    print('wrote %d cases' % len(names))


if __name__ == '__main__':
    main()
