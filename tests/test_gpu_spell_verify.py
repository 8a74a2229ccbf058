"""
GPU tests of DLWP.verify.spells: every verify function on device tensors and device-valued Forecasts equals its host path
exactly -- the integers, and the float64 frequency and mean_length that both paths form from equal integers with one division --
for every threshold kind, a ClimatologyLookup built from climatology_quantiles, both missing modes and a
(f_hour, time, face, height, width) forecast; the results stay on the device and keep their labels.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import spell_ref as S                                                     # noqa: E402
from test_gpu_large_index import poisoned_results                        # noqa: E402,F401  (the fixture is autouse here too)

from DLWP import verify                                                   # noqa: E402
from DLWP.labelled import Forecast                                        # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
INT_FIELDS = ('count', 'rows', 'longest', 'longest_start', 'n_valid', 'n_true')


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _values(r):
    v = r.values if hasattr(r, 'dims') else r
    assert isinstance(v, torch.Tensor) and v.is_cuda, 'the result left the device'
    return v.cpu().numpy()


def _same_everywhere(xh, xd, th, td, **kw):
    """the four functions on the host inputs and on the device inputs: equal, with equal labels"""
    hs, ds = verify.spell_statistics(xh, th, **kw), verify.spell_statistics(xd, td, **kw)
    for k in INT_FIELDS:
        h, d = getattr(hs, k), getattr(ds, k)
        got = _values(d)
        assert got.dtype == np.int32 and np.array_equal(got, getattr(h, 'values', h)), k
        assert getattr(d, 'dims', None) == getattr(h, 'dims', None) and getattr(d, 'name', None) == getattr(h, 'name', None)
    for k in ('frequency', 'mean_length'):
        got = _values(getattr(ds, k))
        want = getattr(getattr(hs, k), 'values', getattr(hs, k))
        assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), np.asarray(want).view(np.uint64)), k
    for fn in (verify.spell_length, verify.spell_position, verify.spell_mask):
        h, d = fn(xh, th, **kw), fn(xd, td, **kw)
        got, want = _values(d), np.asarray(getattr(h, 'values', h))
        assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=fn is verify.spell_mask), fn.__name__
        assert getattr(d, 'dims', None) == getattr(h, 'dims', None) and tuple(got.shape) == tuple(want.shape)
    return hs


@pytest.mark.parametrize('missing', ['break', 'propagate'])
@pytest.mark.parametrize('op', ['>', '>=', '<', '<='])
def test_tensors_equal_the_host_path(op, missing):
    rng = np.random.default_rng(3)
    T, C, H, Wd = 90, 2, 5, 8
    x = (280. + 2. * rng.standard_normal((T, C, H, Wd))).astype(np.float32)
    x[rng.random(x.shape) < 0.01] = np.nan
    x[3, 0, 0, 0] = np.inf
    x[:, 1, 2, :4] = 290.                                               # a spell as long as the series
    kw = dict(op=op, min_length=3, missing=missing)
    _same_everywhere(x, _dev(x), 280., 280., **kw)
    pv = (280. + rng.standard_normal((C, 1, 1))).astype(np.float32)
    _same_everywhere(x, _dev(x), pv, _dev(pv), **kw)
    pg = (280. + rng.standard_normal((1, C, H, Wd))).astype(np.float32)
    pg[0, 0, 1, 1] = np.nan
    _same_everywhere(x, _dev(x), pg, _dev(pg), **kw)
    _same_everywhere(x, _dev(x), pg, pg, **kw)                          # a host threshold goes where the data is
    table = (280. + rng.standard_normal((6, C, H, Wd))).astype(np.float32)
    rows = rng.integers(0, 6, size=T)
    _same_everywhere(x, _dev(x), (table, rows), (_dev(table), rows), **kw)
    y = np.ascontiguousarray(np.moveaxis(x, 0, 2))                      # time on axis 2
    _same_everywhere(y, _dev(y), 280., 280., axis=2, **kw)


def test_a_heat_wave_count_against_a_climatological_quantile():
    """climatology_quantiles(q=0.9) -> a lazy lookup per forecast time -> spell_statistics(min_length=3), on a
    (f_hour, time, face, height, width) forecast: per lead, on the device, equal to the host path"""
    rng = np.random.default_rng(5)
    n_day, F, N = 3 * 365, 2, 4
    times = np.datetime64('2001-01-01') + np.arange(n_day).astype('timedelta64[D]')
    season = 10. * np.sin(2. * np.pi * np.arange(n_day) / 365.25)[:, None, None, None]
    noise = rng.standard_normal((n_day, 6, N, N))
    for t in range(1, n_day):
        noise[t] += 0.7 * noise[t - 1]
    an = (280. + season + 2. * noise).astype(np.float32)
    dims = ('time', 'face', 'height', 'width')
    coords = {'time': times, 'face': np.arange(6), 'height': np.arange(N), 'width': np.arange(N)}
    q_h = verify.climatology_quantiles(Forecast(an, dims, coords), 0.9).isel(quantile=0)
    q_d = Forecast(_dev(q_h.values), q_h.dims, q_h.coords)               # the same table where the forecast lies
    T = 200
    f_hour = np.array([24, 72])
    ft = times[365:365 + T]
    fc = np.stack([an[365 + 1:365 + 1 + T], an[365 + 3:365 + 3 + T]]) + rng.standard_normal((F, T, 6, N, N)).astype(np.float32)
    fc[0, 17, 2, 1, 1] = np.nan
    fdims, fcoords = ('f_hour',) + dims, dict(coords, f_hour=f_hour, time=ft)
    look_h = verify.daily_climo_time_series(q_h, ft, f_hour, lazy=True)
    look_d = verify.daily_climo_time_series(q_d, ft, f_hour, lazy=True)
    assert look_h.rows.shape == (F, T)
    for missing in ('break', 'propagate'):
        hs = _same_everywhere(Forecast(fc, fdims, fcoords), Forecast(_dev(fc), fdims, fcoords), look_h, look_d, min_length=3, missing=missing)
        assert hs.count.dims == ('f_hour', 'face', 'height', 'width') and hs.count.values.max() >= 1
    # one lead against its own row of the lookup, and the laid-out series as an independent statement of the threshold
    series = look_h.materialize().values
    for lead in range(F):
        want = S.reference_vector(fc[lead].reshape(T, -1), series[lead].reshape(T, -1), np.arange(T), S.GT, 3, S.BREAK)[2]
        got = verify.spell_statistics(_dev(fc[lead]), (q_d.values, look_d.rows[lead]), min_length=3)
        assert np.array_equal(_values(got.count).reshape(-1), want[2]) and np.array_equal(_values(got.longest_start).reshape(-1), want[5])


def test_the_mask_feeds_the_bootstrap_and_a_blocking_index():
    """a 0 / 1 blocking index: spells of at least five days; the mask of the blocked days is a series like any other"""
    rng = np.random.default_rng(9)
    T, E = 400, 24
    idx = (rng.random((T, E)) < 0.85).astype(np.float32)
    idx[100:140, 0] = 1.
    hs = _same_everywhere(idx, _dev(idx), 0.5, 0.5, op='>=', min_length=5)
    assert hs.longest[0] >= 40
    mask_d = verify.spell_mask(_dev(idx), 0.5, op='>=', min_length=5)
    iv = verify.bootstrap_interval(mask_d, n_resamples=50, block_length=5)
    assert np.allclose(_values(iv.estimate), hs.frequency, rtol=1e-6)


def test_errors_on_the_device():
    from DLWP import ops
    x = torch.zeros((8, 3), device=DEV)
    for kw in (dict(op='=='), dict(min_length=0), dict(min_length=1.5), dict(missing='skip'), dict(slab_rows=48), dict(statistics=False),
               dict(slab_rows=96, position=True), dict(out_perm=(0, 0))):
        with pytest.raises(ValueError):
            ops.time_spell(x, 0., **kw)
    for thr in (torch.zeros((2, 3), device=DEV), torch.zeros((1, 4), device=DEV), torch.zeros((1, 1, 3), device=DEV)):
        with pytest.raises(ValueError):
            ops.time_spell(x, thr)
    with pytest.raises(ValueError):
        ops.time_spell(x, torch.zeros((2, 3), device=DEV), np.zeros(7, dtype=np.int64))
    with pytest.raises(IndexError):
        ops.time_spell(x, torch.zeros((2, 3), device=DEV), np.full(8, 2))
    for thr in (torch.zeros((1, 3)), torch.zeros((1, 3), device=DEV, dtype=torch.float64), 'hot', None):
        with pytest.raises(TypeError):
            ops.time_spell(x, thr)
    with pytest.raises(TypeError):
        ops.time_spell(x.double(), 0.)
    with pytest.raises(TypeError):
        ops.time_spell(x, torch.zeros((2, 3), device=DEV), torch.zeros(8, device=DEV))
    with pytest.raises(TypeError):
        verify.spell_statistics(x.double(), 0.)
