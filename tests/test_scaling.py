"""
CPU tests of DLWP.model.preprocessing: the host paths of mean_by_batch / std_by_batch against the reference's recorded outputs
(tests/golden/g16_scaling.npz, made by tests/golden/gen_golden_scaling.py), variable_statistics against the fp64 numpy
definition, and VariableScaler against the reference's float32 expressions.
"""
import inspect
import os

import numpy as np
import pytest

import scaling_ref as sr

U = 2.0 ** -24


@pytest.fixture(scope='module')
def g(golden_dir):
    return np.load(os.path.join(golden_dir, 'g16_scaling.npz'))


@pytest.mark.parametrize('axis', [0, 1])
@pytest.mark.parametrize('batch', [1, 8, 100])
def test_host_mean_and_std_by_batch_match_the_reference(g, axis, batch):
    """The reference adds float32 batch sums, the engine fp64: they agree to the reference's own rounding and no further.
    n elements: numpy's blocked pairwise float32 sum carries about log2 n roundings per element, the batch sums, the division and
    (std) the subtraction, the square and the root the rest -- mean within (log2 n + 24) u mean|x|, std within (log2 n + 28) u
    relative, u = 2^-24."""
    from DLWP.model.preprocessing import mean_by_batch, std_by_batch
    x = g['x']
    key = 'axis%d_batch%d' % (axis, batch)
    n = x.size
    mean = mean_by_batch(x, batch, axis)
    assert isinstance(mean, float)
    want = float(g['mean_' + key])
    bound = (np.log2(n) + 24) * U * float(np.abs(x.astype(np.float64)).mean())
    print('mean %r reference %r |diff| %.3e bound %.3e' % (mean, want, abs(mean - want), bound))
    assert abs(mean - want) <= bound
    rel = (np.log2(n) + 28) * U
    for name, kw in (('std_given_', {'mean': want}), ('std_', {})):
        std = std_by_batch(x, batch, axis, **kw)
        assert isinstance(std, float)
        w = float(g[name + key])
        print('%s %r reference %r rel %.3e bound %.3e' % (name, std, w, abs(std - w) / w, rel))
        assert abs(std - w) <= rel * w
    # the engine's own numbers are the fp64 definition
    x64 = x.astype(np.float64)
    assert abs(mean - x64.mean()) <= 1e-13 * abs(x64.mean())
    assert abs(std_by_batch(x, batch, axis) - x64.std()) <= 1e-12 * x64.std()


def test_by_batch_accepts_wrapped_values_and_tensors(g):
    import torch
    from DLWP.model.extensions import Forecast
    from DLWP.model.preprocessing import mean_by_batch, std_by_batch
    x = g['x']
    m = mean_by_batch(x, 8)
    fc = Forecast(x, ('sample', 'varlev', 'face', 'height', 'width'), {})
    assert mean_by_batch(fc, 8) == m and mean_by_batch(torch.from_numpy(x), 8) == m
    assert std_by_batch(fc, 8, mean=m) == std_by_batch(x, 8, mean=m)


def test_reference_signatures():
    from DLWP.model import preprocessing as pp
    assert str(inspect.signature(pp.mean_by_batch)) == '(da, batch_size, axis=0)'
    assert str(inspect.signature(pp.std_by_batch)) == '(da, batch_size, axis=0, mean=None)'
    assert str(inspect.signature(pp.variable_statistics)) == '(array, axis=1, rows=None, skipna=False, center=None)'
    assert str(inspect.signature(pp.VariableScaler.__init__)) == "(self, mean, std, dim='varlev')"
    assert str(inspect.signature(pp.VariableScaler.transform)) == '(self, x, axis=None, out=None)'
    assert str(inspect.signature(pp.VariableScaler.inverse_transform)) == '(self, x, axis=None, out=None, channels_first=False)'
    import DLWP.model as model
    for name in ('VariableScaler', 'mean_by_batch', 'std_by_batch', 'variable_statistics'):
        assert getattr(model, name) is getattr(pp, name)


# ---- variable_statistics ------------------------------------------------------------------------------------------------ #

def _field(seed=3, T=21, V=3, S=(6, 4, 4)):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, V) + S)
    x *= np.array([3., 0.02, 40.])[:V].reshape((1, V) + (1,) * len(S))
    x += np.array([280., -0.5, 1000.])[:V].reshape((1, V) + (1,) * len(S))
    return x.astype(np.float32)


@pytest.mark.parametrize('rows', [None, slice(2, 20, 3), [5, 1, 1, 17, 0]])
@pytest.mark.parametrize('axis', [1, -1])
def test_variable_statistics_is_the_fp64_definition(rows, axis):
    from DLWP.model.preprocessing import variable_statistics
    x = _field()
    if axis == -1:
        x = np.ascontiguousarray(np.moveaxis(x, 1, -1))
    r = None if rows is None else np.arange(x.shape[0])[rows] if isinstance(rows, slice) else np.asarray(rows)
    sel = x if r is None else x[r]
    s64 = np.moveaxis(sel.astype(np.float64), axis, 0).reshape(x.shape[axis], -1)
    mean, std = variable_statistics(x, axis=axis, rows=r)
    assert mean.dtype == np.float64 and std.dtype == np.float64 and mean.shape == (3,)
    np.testing.assert_allclose(mean, s64.mean(axis=1), rtol=1e-13)
    np.testing.assert_allclose(std, s64.std(axis=1), rtol=1e-12)
    # one pass around an approximate mean: same numbers up to the cancellation the docstring names
    m1, s1 = variable_statistics(x, axis=axis, rows=r, center=np.round(mean))
    np.testing.assert_allclose(m1, mean, rtol=1e-13)
    np.testing.assert_allclose(s1, std, rtol=1e-9)


def test_variable_statistics_nan_policy():
    from DLWP.model.preprocessing import variable_statistics
    x = _field(seed=4)
    x[0, 0, 0, 0, 0] = np.nan
    x[3, 0] = np.nan
    x[-1, 2, -1, -1, -1] = np.nan
    mean, std = variable_statistics(x)
    assert np.isnan(mean[[0, 2]]).all() and np.isnan(std[[0, 2]]).all() and np.isfinite(mean[1]) and np.isfinite(std[1])
    mean, std = variable_statistics(x, skipna=True)
    s64 = np.moveaxis(x.astype(np.float64), 1, 0).reshape(3, -1)
    np.testing.assert_allclose(mean, np.nanmean(s64, axis=1), rtol=1e-13)
    np.testing.assert_allclose(std, np.nanstd(s64, axis=1), rtol=1e-12)
    with pytest.raises(ValueError):
        variable_statistics(x, axis=0, rows=[0, 1])


# ---- VariableScaler ----------------------------------------------------------------------------------------------------- #

MEAN = np.array([280.25, -0.5, 1000.125], dtype=np.float32)
STD = np.array([3.1, 0.02, 41.7], dtype=np.float32)


def test_scaler_on_numpy_is_the_reference_float32_arithmetic():
    from DLWP.model.preprocessing import VariableScaler
    x = _field(seed=5)
    sc = VariableScaler(MEAN, STD)
    assert sc.mean.dtype == np.float32 and sc.std.dtype == np.float32 and len(sc) == 3
    y = sc.transform(x)
    want = np.empty_like(x)
    for v in range(3):                                      # preprocessing.py:660, one variable at a time in float32
        want[:, v] = (x[:, v] - MEAN[v]) / STD[v]
    assert y.dtype == np.float32 and sr.same_bits(y, want) and sr.same_bits(y, sr.affine(x, STD, MEAN, sr.SUB_DIV))
    cl = np.ascontiguousarray(np.moveaxis(y, 1, -1))
    back = sc.inverse_transform(cl, axis=-1)
    assert sr.same_bits(back, cl * STD + MEAN)              # Tutorial 4, cell 19
    # round trip: (x - m) / s * s + m returns x within the roundings of the four operations, each at most half an ulp of its
    # result: |x - m| (2 u) from the division and the product, u (|x - m| + |x|) from the subtraction and the sum
    xl = np.moveaxis(x, 1, -1).astype(np.float64)
    bound = U * (3 * np.abs(xl - MEAN.astype(np.float64)) + 2 * np.abs(xl)) * 1.01
    assert np.all(np.abs(back.astype(np.float64) - xl) <= bound)
    # in place, and into a given buffer
    z = x.copy()
    assert sc.transform(z, out=z) is z and sr.same_bits(z, want)
    buf = np.empty_like(cl)
    assert sc.inverse_transform(cl, axis=-1, out=buf) is buf and sr.same_bits(buf, back)


def test_scaler_on_a_forecast_carries_dims_and_moves_the_variable_axis():
    from DLWP.model.extensions import Forecast
    from DLWP.model.preprocessing import VariableScaler
    rng = np.random.default_rng(6)
    vals = rng.standard_normal((4, 5, 6, 2, 2, 3)).astype(np.float32)
    dims = ('f_hour', 'time', 'x0', 'x1', 'x2', 'varlev')
    coords = {'f_hour': np.arange(6, 30, 6), 'time': np.arange(5), 'varlev': np.array(['z', 't', 'u'])}
    fc = Forecast(vals, dims, coords)
    sc = VariableScaler(MEAN, STD)
    out = sc.inverse_transform(fc)
    assert isinstance(out, Forecast) and out.dims == dims and out.coords.keys() == coords.keys()
    assert sr.same_bits(out.values, vals * STD + MEAN) and sr.same_bits(fc.values, vals)
    cf = sc.inverse_transform(fc, channels_first=True)
    assert cf.dims == ('f_hour', 'time', 'varlev', 'x0', 'x1', 'x2') and cf.values.shape == (4, 5, 3, 6, 2, 2)
    assert cf.values.flags['C_CONTIGUOUS'] and sr.same_bits(cf.values, (vals * STD + MEAN).transpose(0, 1, 5, 2, 3, 4))
    assert np.array_equal(cf.coords['varlev'], coords['varlev'])
    again = sc.transform(cf)                                # the axis is found by name wherever it is
    assert again.dims == cf.dims and sr.same_bits(again.values, sr.affine(cf.values, STD, MEAN, sr.SUB_DIV, axis=2))
    # a plain array: to position 2, or to the position asked for
    assert sr.same_bits(sc.inverse_transform(vals, axis=-1, channels_first=True), cf.values)
    assert sc.inverse_transform(vals, axis=-1, channels_first=1).shape == (4, 3, 5, 6, 2, 2)


def test_scaler_fit_sel_and_errors():
    from DLWP.model.preprocessing import VariableScaler, variable_statistics
    x = _field(seed=7)
    rows = np.arange(0, 15)
    sc = VariableScaler.fit(x, rows=rows)
    mean, std = variable_statistics(x, rows=rows)
    assert np.array_equal(sc.mean, mean.astype(np.float32)) and np.array_equal(sc.std, std.astype(np.float32))
    sub = sc.sel([2, 0])
    assert np.array_equal(sub.mean, sc.mean[[2, 0]]) and np.array_equal(sub.std, sc.std[[2, 0]]) and sub.dim == sc.dim
    assert sr.same_bits(sub.transform(x[:, [2, 0]]), sc.transform(x)[:, [2, 0]])
    for bad in ([1., 0., 2.], [1., np.inf, 2.], [1., np.nan, 2.], [1., 1e-50, 2.]):
        with pytest.raises(ValueError):
            VariableScaler([0., 0., 0.], bad)
    with pytest.raises(ValueError):
        VariableScaler([0., 0.], [1., 1., 1.])
    with pytest.raises(ValueError, match='2 variables.*scaler 3'):
        sc.transform(x[:, :2])
    with pytest.raises(ValueError):
        sc.transform(x, out=np.empty((2, 2), np.float32))


@pytest.mark.parametrize('first', ['DLWP.verify', 'DLWP.model.preprocessing', 'DLWP.model.extensions'])
def test_each_module_can_be_a_process_first_import(first):
    """DLWP.verify and DLWP.model.preprocessing both take the labelled-array helpers from the leaf DLWP.labelled, and neither
    imports the other at module level: whichever a fresh process imports first, no module may need a name of one that is only
    half initialised"""
    import subprocess
    import sys
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'dlwp-cs_amd')
    code = ('import sys; sys.path.insert(0, %r); import %s; from DLWP.verify import forecast_error; '
            'from DLWP.model import VariableScaler, mean_by_batch, std_by_batch, variable_statistics' % (pkg, first))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
