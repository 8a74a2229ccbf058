"""
Solar forcing described instead of stored (DLWP.util.SolarForcing, dlwpcs_solar_fill): the host side.

  * The two tables the device computes from, pushed through the kernel's arithmetic restated in numpy (tests/solar_ref.py, numpy's
    own fp32 cosine), give DLWP.util.insolation BIT FOR BIT.  That pins the tables and the order of the operations; the goldens
    (tests/golden/g6_insolation.npz, test_generators.py) already pin DLWP.util.insolation to the reference.
    (The kernel multiplies by scale = S * dist**-2 where the host function multiplies by S and then by dist**-2: two fp64 roundings
    in another order, below what the rounding to fp32 keeps for every element of these cases.)
  * The lazy object behaves like the dense array it stands for: rows, np.asarray, its continuation past the dates.
  * The host generator and the estimator's host loop fed the lazy object give bitwise what they give for the dense array, and the
    estimator no longer stops at the end of the generator's rows.
"""
import os

import numpy as np
import pandas as pd
import pytest

import solar_ref as SR
from test_estimator import ITS, _StubNet, host_device  # noqa: F401  (the fixture)


def _sf(*a, **kw):
    from DLWP.util import SolarForcing
    return SolarForcing(*a, **kw)


def _check_tables(dates, lat, lon, **kw):
    from DLWP.util import insolation
    ref = insolation(dates, lat, lon, **kw)
    sf = _sf(dates, lat, lon, **kw)
    assert sf.row_table.shape == (len(dates), 4) and sf.row_table.dtype == np.float64
    assert sf.cell_table.shape == (ref[0].size, 3) and sf.cell_table.dtype == np.float64
    # day and lon / 360 are fp32 values carried in fp64
    assert np.array_equal(sf.row_table[:, 3], sf.row_table[:, 3].astype(np.float32).astype(np.float64))
    assert np.array_equal(sf.cell_table[:, 2], sf.cell_table[:, 2].astype(np.float32).astype(np.float64))
    got = SR.fill(sf.row_table, sf.cell_table, np.arange(len(dates))).reshape(ref.shape)
    assert got.dtype == np.float32
    assert np.array_equal(got.view(np.int32), ref.view(np.int32))
    assert sf.shape == ref.shape and sf.dtype == ref.dtype and len(sf) == len(ref) and sf.ndim == ref.ndim
    return sf, ref


def test_tables_reproduce_the_host_function_on_the_golden_inputs(golden_dir):
    g = np.load(os.path.join(golden_dir, 'g6_insolation.npz'))
    dates = pd.to_datetime(list(g['dates']))
    _check_tables(dates, g['lat1'], g['lon1'])
    _check_tables(dates, g['lat2'], g['lon2'], S=1361.)
    _check_tables(dates, g['lat1'], g['lon1'], daily=True)
    _check_tables(dates, g['lat2'], g['lon2'], S=1361., daily=True)


@pytest.mark.parametrize('case', sorted(SR.DATE_CASES))
@pytest.mark.parametrize('daily', [False, True])
@pytest.mark.parametrize('S', [1., 1361., 0.37])
def test_tables_reproduce_the_host_function_on_the_cubed_sphere(case, daily, S):
    lat, lon = SR.cube_latlon(8)
    start, n = SR.DATE_CASES[case]
    _check_tables(SR.dates_6h(start, n), lat, lon, S=S, daily=daily)
    _check_tables(SR.dates_6h(start, n), lat.astype(np.float32), lon.astype(np.float32), S=S, daily=daily)


def test_daily_is_only_another_table():
    lat, lon = SR.cube_latlon(4)
    dates = SR.dates_6h('2016-02-27T00', 12)
    a, b = _sf(dates, lat, lon), _sf(dates, lat, lon, daily=True)
    assert np.array_equal(a.cell_table[:, :2], b.cell_table[:, :2]) and not b.cell_table[:, 2].any()
    assert np.array_equal(b.row_table[:, 3], 0.5 + np.round(a.row_table[:, 3]))


def test_lazy_object_is_the_dense_array():
    from DLWP.util import insolation
    lat, lon = SR.cube_latlon(4)
    dates = SR.dates_6h('2015-12-30T00', 20)
    sf = _sf(dates, lat, lon, S=2.5)
    dense = insolation(dates, lat, lon, S=2.5)
    assert np.array_equal(np.asarray(sf), dense) and np.asarray(sf).dtype == np.float32
    assert np.asarray(sf, dtype=np.float64).dtype == np.float64
    for key in (3, -1, slice(2, 9), slice(None, None, 3), np.array([7, 0, 7, 19]), np.array([[1, 2], [5, 4]]), [4, 5],
                np.arange(20) % 3 == 0, slice(5, 5)):
        assert np.array_equal(sf[key], dense[key]), key
    assert np.array_equal(sf[np.array([1, 6]), 2], dense[np.array([1, 6]), 2])
    assert np.array_equal(sf[4, 1, :, 2], dense[4, 1, :, 2])
    with pytest.raises(IndexError):
        sf[20]
    with pytest.raises(IndexError):
        sf[np.array([0, 25])]
    assert sf.nbytes == (20 * 4 + 6 * 4 * 4 * 3) * 8


def test_rows_continue_the_record_past_its_dates():
    from DLWP.util import insolation
    lat, lon = SR.cube_latlon(4)
    dates = SR.dates_6h('2016-12-25T00', 16)
    sf = _sf(dates, lat, lon)
    assert sf.rows(16) is sf and sf.rows(3) is sf
    more = sf.rows(41)
    assert len(more) >= 41 and more.rows(30) is more and sf.rows(35) is more          # one continuation serves the shorter asks
    ext = SR.dates_6h('2016-12-25T00', len(more))
    dense = insolation(ext, lat, lon)
    assert np.array_equal(np.asarray(more), dense)
    assert np.array_equal(SR.fill(more.row_table, more.cell_table, np.arange(len(more))).reshape(dense.shape), dense)
    assert np.array_equal(more.row_table[:16], sf.row_table) and np.array_equal(more.cell_table, sf.cell_table)
    # an explicit time step; a single date has none
    daily = _sf(dates[:1], lat, lon, dt=np.timedelta64(1, 'D')).rows(3)
    assert np.array_equal(np.asarray(daily)[:3], insolation(SR.dates_6h('2016-12-25T00', 3, hours=24), lat, lon))
    with pytest.raises(IndexError):
        _sf(dates[:1], lat, lon).rows(2)


class _Meta(object):
    is_convolutional, is_recurrent, impute = True, False, False


GEN_CASES, gen_data = SR.GEN_CASES, SR.gen_data


@pytest.mark.parametrize('name', sorted(GEN_CASES))
def test_host_generator_takes_the_lazy_object(name):
    from DLWP.model.generators import ArrayDataGenerator
    arr, const, sf = gen_data()
    dense = np.asarray(sf)
    kw = dict(rank=3, batch_size=5, constants=const, **GEN_CASES[name])
    a = ArrayDataGenerator(_Meta(), arr, insolation_array=dense, **kw)
    b = ArrayDataGenerator(_Meta(), arr, insolation_array=sf, **kw)
    assert len(a) == len(b) and a.convolution_shape == b.convolution_shape and a.insolation_shape == b.insolation_shape
    for index in (0, 2, len(a) - 1):
        (pa, ta), (pb, tb) = a[index], b[index]
        flat = lambda x: list(x) if isinstance(x, (list, tuple)) else [x]   # noqa: E731
        assert len(flat(pa)) == len(flat(pb)) and len(flat(ta)) == len(flat(tb))
        for x, y in zip(flat(pa) + flat(ta), flat(pb) + flat(tb)):
            assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y)
    with pytest.raises(IndexError):
        b.generate([len(arr)])


def _estimators(n_out=2):
    from DLWP.model import DLWPFunctional, TimeSeriesEstimator
    from DLWP.model.generators import ArrayDataGenerator
    arr, const, sf = gen_data(N=4, T=40, V=3)
    out = []
    for sol in (np.asarray(sf), sf):
        dlwp = DLWPFunctional(is_convolutional=True, time_dim=ITS)
        dlwp.build_model(_StubNet(n_out), loss='mse')
        gen = ArrayDataGenerator(dlwp, arr, rank=3, batch_size=4, input_time_steps=ITS, output_time_steps=ITS, sequence=n_out,
                                 insolation_array=sol, constants=const, channels_last=True)
        out.append(TimeSeriesEstimator(dlwp, gen))
    return out + [arr, const, sf]


def test_estimator_host_loop_runs_past_the_generators_rows(host_device):  # noqa: F811
    from DLWP.util import insolation
    dense_est, lazy_est, arr, const, sf = _estimators()
    # over the rows both can serve: the same bits
    samples = np.array([0, 3, 5])
    a, b = dense_est.predict(8, samples=samples), lazy_est.predict(8, samples=samples)
    assert np.array_equal(a.values, b.values) and a.dims == b.dims
    # 40 steps from row 30 read insolation far past row 39: the dense array (no times given) stops, the description goes on
    with pytest.raises(IndexError):
        dense_est.predict(40, samples=[30])
    fc = lazy_est.predict(40, samples=[30, 12])
    assert fc.values.shape[:2] == (40, 2) and np.isfinite(fc.values).all()
    # ... and what it computes there is the forecast of an estimator that was handed the long dense array
    from DLWP.model import DLWPFunctional, TimeSeriesEstimator
    from DLWP.model.generators import ArrayDataGenerator
    need = len(sf.rows(30 + 10 * ITS * 2 + 2 * ITS))
    long_sol = insolation(SR.dates_6h('2015-12-27T00', need), sf.lat, sf.lon)
    dlwp = DLWPFunctional(is_convolutional=True, time_dim=ITS)
    dlwp.build_model(_StubNet(2), loss='mse')
    gen = ArrayDataGenerator(dlwp, arr, rank=3, batch_size=4, input_time_steps=ITS, output_time_steps=ITS, sequence=2,
                             insolation_array=long_sol[:40], constants=const, channels_last=True)
    gen.insolation_array = long_sol                               # (the estimator reads it; the generator's batches stay in range)
    ref = TimeSeriesEstimator(dlwp, gen).predict(40, samples=[30, 12])
    assert np.array_equal(fc.values, ref.values)
