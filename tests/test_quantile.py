"""
DLWP.verify.climatology_quantiles on the host path (numpy, interpolated in float64) against quantile_ref.py: bits, labels, dims
and coordinates, `by` in its three forms, the round trip through daily_climo_time_series, and every refusal -- those of the
device path included, which the plan query answers on the host.  No device work.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import quantile_ref as R     # noqa: E402

from DLWP import verify as V                         # noqa: E402
from DLWP.model.extensions import Forecast          # noqa: E402

TERCILES = (1. / 3., 2. / 3.)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _series(rng, n_time=3 * 366, dims=('time', 'face', 'varlev'), shape=(4, 8), start='2003-01-01'):
    """daily data over three years with every kind of column of the input maker"""
    times = np.datetime64(start) + np.arange(n_time).astype('timedelta64[D]')
    x, _ = R.make_columns(rng, n_time, int(np.prod(shape)))
    t_ax = dims.index('time')
    v = np.moveaxis(x.reshape((n_time,) + shape), 0, t_ax)
    coords = {d: (times if d == 'time' else np.arange(n) * 2.0) for d, n in zip(dims, v.shape)}
    return Forecast(np.ascontiguousarray(v), dims, coords), x, times


def _reference(x, keys, probs):
    uniq, start, order = V._csr(keys)
    q, c = R.reference(x, start, order, probs)
    return q, c, uniq


@pytest.mark.parametrize('by', ['dayofyear', 'month', None])
def test_values_are_the_reference_bit_for_bit(by):
    rng = np.random.default_rng(1)
    ds, x, times = _series(rng)
    probs = (0., 0.1) + TERCILES + (1.,)
    keys = np.zeros(len(times), dtype=np.int64) if by is None else V.calendar_keys(times, by)
    q, _, uniq = _reference(x, keys, probs)
    out = V.climatology_quantiles(ds, probs, by=by)
    assert isinstance(out, Forecast) and out.values.dtype == np.float32 and out.name == 'climatology_quantiles'
    if by is None:
        assert out.dims == ('quantile', 'face', 'varlev') and out.values.shape == (5, 4, 8)
        assert np.array_equal(_bits(out.values), _bits(q[:, 0].reshape(5, 4, 8)))
    else:
        assert out.dims == ('quantile', by, 'face', 'varlev') and out.values.shape == (5, len(uniq), 4, 8)
        assert np.array_equal(out.coords[by], uniq) and out.coords[by].dtype == np.int64
        assert np.array_equal(_bits(out.values), _bits(q.reshape(5, len(uniq), 4, 8)))
    assert np.array_equal(out.coords['quantile'], probs) and np.array_equal(out.coords['face'], ds.coords['face'])
    assert len(uniq) == {'dayofyear': 366, 'month': 12, None: 1}[by]


def test_time_on_any_axis_and_a_scalar_probability():
    rng = np.random.default_rng(2)
    ds, x, times = _series(rng, n_time=400, dims=('face', 'time', 'varlev'), shape=(3, 5))
    q, _, uniq = _reference(x, V.calendar_keys(times, 'month'), (0.5,))
    out = V.climatology_quantiles(ds, 0.5, by='month')
    assert out.dims == ('quantile', 'face', 'month', 'varlev') and out.values.shape == (1, 3, 12, 5)
    assert np.array_equal(_bits(out.values), _bits(np.moveaxis(q.reshape(1, 12, 3, 5), 1, 2)))
    ds.lat = 'kept'
    assert V.climatology_quantiles(ds, 0.5, by=None).lat == 'kept'


def test_host_formula_is_the_reference_on_every_group_length():
    rng = np.random.default_rng(3)
    for rows in (1, 2, 3, 65, 300):
        x, _ = R.make_columns(rng, rows, 40, shift=rows)
        gs, ri = R.make_groups(rng, rows, (rows, 0, max(rows // 2, 1)))
        probs = R.GPU_PROBS[5]
        q, c = R.reference(x, gs, ri, probs)
        got = V._group_quantile_host(x, 0, gs, ri, probs)
        assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(q)), rows
        # the row axis last, and an output permutation
        got = V._group_quantile_host(np.ascontiguousarray(x.T), 1, gs, ri, probs, out_perm=(1, 0))
        assert np.array_equal(_bits(got), _bits(q)), rows


def test_round_trip_through_the_climatology_time_series():
    """a quantile table by day of the year laid out along forecast times: daily_climo_time_series finds 'dayofyear' by name"""
    rng = np.random.default_rng(4)
    ds, x, times = _series(rng, dims=('time', 'face', 'varlev'))
    table = V.climatology_quantiles(ds, TERCILES)
    when = np.array(['2005-03-01', '2004-02-29', '2007-12-31'], dtype='datetime64[D]')
    f_hour = np.array([0, 24, 48])
    for lazy in (False, True):
        series = V.daily_climo_time_series(table, when, f_hour, lazy=lazy)
        assert series.dims == ('f_hour', 'quantile', 'time', 'face', 'varlev') and tuple(series.shape) == (3, 2, 3, 4, 8)
        if lazy:
            series = series.materialize()
        doy = V.calendar_keys(when[None, :] + f_hour[:, None].astype('timedelta64[h]'), 'dayofyear')
        for f in range(3):
            for t in range(3):
                row = int(np.nonzero(table.coords['dayofyear'] == doy[f, t])[0][0])
                assert np.array_equal(_bits(series.values[f, :, t]), _bits(table.values[:, row]))
        assert np.array_equal(series.coords['quantile'], TERCILES)


def test_terciles_split_a_long_series_in_three():
    rng = np.random.default_rng(5)
    n = 3000
    v = rng.standard_normal((n, 6)).astype(np.float32)
    ds = Forecast(v, ('time', 'x'), {'time': np.datetime64('2000-01-01') + np.arange(n).astype('timedelta64[D]'), 'x': np.arange(6)})
    t = V.climatology_quantiles(ds, TERCILES, by=None).values
    below = (v[None] <= t[:, None]).mean(axis=1)
    assert np.abs(below - np.array(TERCILES)[:, None]).max() <= 1.0 / n + 1e-12
    assert np.allclose(t, np.quantile(v.astype(np.float64), TERCILES, axis=0), rtol=0, atol=1e-6)


def test_refusals():
    rng = np.random.default_rng(6)
    ds, _, _ = _series(rng, n_time=40)
    with pytest.raises(ValueError, match=r'\[0, 1\]'):
        V.climatology_quantiles(ds, (0.5, 1.5))
    with pytest.raises(ValueError, match=r'\[0, 1\]'):
        V.climatology_quantiles(ds, (np.nan,))
    with pytest.raises(ValueError, match='probabilities'):
        V.climatology_quantiles(ds, np.linspace(0, 1, 17))
    with pytest.raises(ValueError, match='probabilities'):
        V.climatology_quantiles(ds, ())
    with pytest.raises(ValueError, match="'by'"):
        V.climatology_quantiles(ds, 0.5, by='week')
    with pytest.raises(ValueError, match="'time'"):
        V.climatology_quantiles(Forecast(np.zeros((3, 2), np.float32), ('a', 'b'), {}), 0.5)
    with pytest.raises(TypeError, match='datetime64'):
        V.climatology_quantiles(Forecast(np.zeros((3, 2), np.float32), ('time', 'b'), {'time': np.arange(3)}), 0.5)
    with pytest.raises(ValueError, match='entries'):
        V.climatology_quantiles(Forecast(np.zeros((3, 2), np.float32), ('time', 'b'), {'time': ds.coords['time'][:2]}), 0.5)


def test_device_path_refusals_answered_on_the_host():
    import torch
    from DLWP import _native as nat
    from DLWP import ops
    assert ops.QUANTILE_MAX_PROBS == R.MAX_PROBS == 16
    with pytest.raises(ValueError, match=r'\[0, 1\]'):
        ops.group_quantile(torch.zeros(4, 8), [0, 4], np.arange(4), (0.2, -0.1))
    with pytest.raises(ValueError, match='probabilities'):
        ops.group_quantile(torch.zeros(4, 8), [0, 4], np.arange(4), np.linspace(0, 1, 17))
    with pytest.raises(ValueError, match='group_start'):
        ops.group_quantile(torch.zeros(4, 8), [0, 3], np.arange(4), (0.5,))
    with pytest.raises(IndexError):
        ops.group_quantile(torch.zeros(4, 8), [0, 4], np.arange(1, 5), (0.5,))
    with pytest.raises(nat.NativeError):
        ops.group_quantile(torch.zeros(4, 8), [0, 4], np.arange(4), (0.5,))           # no CPU fallback behind the device entry
    lib = nat.lib()
    import ctypes
    d, _ = ops.rows_layout((4, 8), (8, 1), 0, None, 1)
    p = (ctypes.c_double * 2)(0.5, 1.0 + 1e-9)
    assert lib.dlwpcs_group_quantile(ctypes.byref(d), 256, 512, 768, 1, 4, p, 2, 1024, 8, None, None) == -1
    assert b'outside [0, 1]' in lib.dlwpcs_last_error()
    assert lib.dlwpcs_group_quantile(ctypes.byref(d), 256, 512, 768, 1, 4, p, 17, 1024, 8, None, None) == -1
    assert lib.dlwpcs_group_quantile(ctypes.byref(d), 256, 512, 768, 0, 4, p, 1, 1024, 8, None, None) == 0       # no group: no launch
