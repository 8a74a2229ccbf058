"""
How DLWP.verify labels its results and resolves its axes, written out per public function: the dims of the result, which
coordinates it has and the values of those that are new, the result's name, whether `.lat` rides along -- the families differ in
that, and the difference is pinned here as it is -- and the exact message of every axis error.  Host paths only; the values
themselves are the business of the family tests.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from DLWP import verify as V
from DLWP.model.extensions import Forecast

LAT = np.array([-67.5, -22.5, 22.5, 67.5])
TIMES = np.datetime64('2001-01-01') + np.arange(8) * np.timedelta64(1, 'D')
LON = np.arange(6) * 60.0
DAYS = np.arange(1, 9)
BASIS = np.stack([np.ones(8), np.linspace(-1., 1., 8)], axis=1)
TAPS = np.ones(3) / 3.


def _array(seed=0):
    return np.random.default_rng(seed).normal(size=(8, 4, 6))


def _field(seed=0):
    """(time, lat, lon) with coordinates on time and lat only, and a `.lat` attribute"""
    f = Forecast(_array(seed), ('time', 'lat', 'lon'), {'time': TIMES, 'lat': LAT}, name='x')
    f.lat = LAT
    return f


def _ensemble():
    return V.stack_forecasts([_field(s) for s in range(3)])


def _quartiles():
    return Forecast(np.array([-0.5, 0.5]), ('quantile',), {'quantile': np.array([0.25, 0.75])}, name='q')


def _check(res, dims, coords, name, lat):
    assert isinstance(res, Forecast)
    assert res.dims == tuple(dims)
    assert tuple(res.values.shape) == tuple(np.shape(res.values)) and len(res.values.shape) == len(dims)
    assert set(res.coords) == set(coords)
    for d, c in coords.items():
        got = np.asarray(res.coords[d])
        assert got.shape == np.shape(c) and np.array_equal(got, c), d
        assert got.shape[0] == res.values.shape[res.dims.index(d)], d
    assert res.name == name
    assert hasattr(res, 'lat') == lat
    if lat:
        assert res.lat is LAT


TL = {'time': TIMES, 'lat': LAT}


# --------------------------------------------------------------------------------------------------------------------- #
# climatologies: `.lat` rides along on the tables, not on the series laid out from them
# --------------------------------------------------------------------------------------------------------------------- #

def test_climatology_tables():
    x = _field()
    _check(V.daily_climatology(x), ('dayofyear', 'lat', 'lon'), {'dayofyear': DAYS, 'lat': LAT}, 'climatology', True)
    _check(V.daily_climatology(x, by='month'), ('month', 'lat', 'lon'), {'month': np.array([1]), 'lat': LAT}, 'climatology', True)
    q = np.array([1. / 3., 2. / 3.])
    _check(V.climatology_quantiles(x, q), ('quantile', 'dayofyear', 'lat', 'lon'), {'quantile': q, 'dayofyear': DAYS, 'lat': LAT},
           'climatology_quantiles', True)
    _check(V.climatology_quantiles(x, 0.5, by=None), ('quantile', 'lat', 'lon'), {'quantile': np.array([0.5]), 'lat': LAT},
           'climatology_quantiles', True)


def test_climatology_series_and_anomaly():
    x = _field()
    clim = V.daily_climatology(x)
    _check(V.daily_climo_time_series(clim, TIMES[:3]), ('time', 'lat', 'lon'), {'time': TIMES[:3], 'lat': LAT}, 'climatology', False)
    lazy = V.daily_climo_time_series(clim, TIMES[:3], f_hour=[0, 24], lazy=True)
    assert lazy.dims == ('f_hour', 'time', 'lat', 'lon') and set(lazy.coords) == {'f_hour', 'time', 'lat'}
    _check(lazy.materialize(), ('f_hour', 'time', 'lat', 'lon'), {'f_hour': np.array([0, 24]), 'time': TIMES[:3], 'lat': LAT},
           'climatology', False)
    _, anomaly = V.monthly_climo_error(x, TIMES[[1, 3]], return_da=True)
    _check(anomaly, ('time', 'lat', 'lon'), {'time': TIMES[[1, 3]], 'lat': LAT}, 'anomaly', False)


# --------------------------------------------------------------------------------------------------------------------- #
# zonal and spherical spectra, analysis and synthesis: no `.lat`
# --------------------------------------------------------------------------------------------------------------------- #

def test_zonal():
    x, y = _field(), _field(1)
    k = np.arange(4)
    _check(V.zonal_spectrum(x), ('wavenumber',), {'wavenumber': k}, 'zonal_spectrum', False)
    _check(V.zonal_spectrum(x, axis='time', n_wave=3), ('lat', 'wavenumber'), {'lat': LAT, 'wavenumber': k[:3]}, 'zonal_spectrum', False)
    res, skipped = V.zonal_spectrum(x, axis=1, return_count=True)
    _check(res, ('time', 'wavenumber'), {'time': TIMES, 'wavenumber': k}, 'zonal_spectrum', False)
    assert type(skipped) is np.ndarray
    cross = V.zonal_cross_spectrum(x, y, axis=('time',))
    for part, name in zip(cross, ('power_f', 'power_v', 'co', 'quad')):
        _check(part, ('lat', 'wavenumber'), {'lat': LAT, 'wavenumber': k}, name, False)
    _check(V.zonal_coherence(x, y, axis=0), ('lat', 'wavenumber'), {'lat': LAT, 'wavenumber': k}, 'zonal_coherence', False)


def test_spherical_spectra():
    x, y = _field(), _field(1)
    n = np.arange(2)
    _check(V.spherical_spectrum(x), ('degree',), {'degree': n}, 'spherical_spectrum', False)
    res, skipped = V.spherical_spectrum(x, axis=(), return_count=True)
    _check(res, ('time', 'degree'), {'time': TIMES, 'degree': n}, 'spherical_spectrum', False)
    assert type(skipped) is np.ndarray
    for part, name in zip(V.spherical_cross_spectrum(x, y, axis=()), ('power_f', 'power_v', 'co')):
        _check(part, ('time', 'degree'), {'time': TIMES, 'degree': n}, name, False)
    _check(V.spherical_correlation(x, y), ('degree',), {'degree': n}, 'spherical_correlation', False)


def test_spherical_fields_and_coefficients():
    x = _field()
    coef = V.spherical_analysis(x)
    _check(coef, ('time', 'coefficient'), {'time': TIMES}, 'spherical_analysis', False)
    assert coef.values.shape == (8, 3)
    grid = {'time': TIMES, 'lat': LAT, 'lon': LON}
    _check(V.spherical_synthesis(coef, LAT, 6), ('time', 'lat', 'lon'), grid, 'spherical_synthesis', False)
    _check(V.spherical_filter(x, cutoff=1), ('time', 'lat', 'lon'), TL, 'spherical_filter', False)
    _check(V.spherical_laplacian(x), ('time', 'lat', 'lon'), TL, 'spherical_laplacian', False)
    for part, name in zip(V.spherical_gradient(x), ('gradient_lon', 'gradient_lat')):
        _check(part, ('time', 'lat', 'lon'), TL, name, False)
    vrt, div = V.spherical_vrtdiv(x, _field(1))
    _check(vrt, ('time', 'coefficient'), {'time': TIMES}, 'vorticity', False)
    _check(div, ('time', 'coefficient'), {'time': TIMES}, 'divergence', False)
    for part, name in zip(V.spherical_uv(vrt, div, LAT, 6), ('u', 'v')):
        _check(part, ('time', 'lat', 'lon'), grid, name, False)
    u, _ = V.spherical_uv(None, div, LAT[::-1], 6)
    _check(u, ('time', 'lat', 'lon'), {'time': TIMES, 'lat': LAT[::-1], 'lon': LON}, 'u', False)


# --------------------------------------------------------------------------------------------------------------------- #
# ensembles: the stacked record and the categorical scores carry `.lat`, the per-element ensemble statistics do not
# --------------------------------------------------------------------------------------------------------------------- #

def test_ensemble():
    ens, y = _ensemble(), _field(5)
    _check(ens, ('member', 'time', 'lat', 'lon'), {'member': np.arange(3), 'time': TIMES, 'lat': LAT}, 'x', True)
    _check(V.ensemble_mean(ens), ('time', 'lat', 'lon'), TL, 'ensemble_mean', False)
    _check(V.ensemble_spread(ens), ('time', 'lat', 'lon'), TL, 'ensemble_spread', False)
    _check(V.ensemble_crps(ens, y), ('time', 'lat', 'lon'), TL, 'ensemble_crps', False)
    _check(V.rank_histogram(ens, y), ('rank',), {'rank': np.arange(4)}, 'rank_histogram', False)
    _check(V.rank_histogram(ens, y, axis=(0, 2)), ('lat', 'rank'), {'lat': LAT, 'rank': np.arange(4)}, 'rank_histogram', False)
    # the member dim need not lead: the positions of `axis` count the dims without it
    mid = Forecast(np.moveaxis(ens.values, 0, 2), ('time', 'lat', 'member', 'lon'), ens.coords, name='x')
    _check(V.ensemble_mean(mid), ('time', 'lat', 'lon'), TL, 'ensemble_mean', False)
    _check(V.rank_histogram(mid, y, axis=(1, 2)), ('time', 'rank'), {'time': TIMES, 'rank': np.arange(4)}, 'rank_histogram', False)


def test_category():
    ens, y = _ensemble(), _field(5)
    bare = [-0.5, 0.5]
    thr = dict(TL, threshold=np.arange(2))
    _check(V.ensemble_probability(ens, bare), ('threshold', 'time', 'lat', 'lon'), thr, 'ensemble_probability', True)
    _check(V.ensemble_probability(ens, _quartiles()), ('quantile', 'time', 'lat', 'lon'), dict(TL, quantile=np.array([0.25, 0.75])),
           'ensemble_probability', True)
    _check(V.brier_score(ens, y, bare), ('threshold', 'time', 'lat', 'lon'), thr, 'brier_score', True)
    _check(V.brier_score(ens, y, _quartiles()), ('quantile', 'time', 'lat', 'lon'), dict(TL, quantile=np.array([0.25, 0.75])),
           'brier_score', True)
    _check(V.ranked_probability_score(ens, y, bare), ('time', 'lat', 'lon'), TL, 'ranked_probability_score', True)
    tail = {'threshold': np.arange(2), 'members_below': np.arange(4), 'observed': np.arange(2)}
    _check(V.reliability_counts(ens, y, bare), ('threshold', 'members_below', 'observed'), tail, 'reliability_counts', True)
    # the last dim is named 'threshold' whatever the thresholds' own dim; its coordinate is theirs
    _check(V.reliability_counts(ens, y, _quartiles(), axis=(0, 2)), ('lat', 'threshold', 'members_below', 'observed'),
           dict(tail, lat=LAT, threshold=np.array([0.25, 0.75])), 'reliability_counts', True)


# --------------------------------------------------------------------------------------------------------------------- #
# along time: filters, fits and spectra carry `.lat`; the counts of the spectra do not
# --------------------------------------------------------------------------------------------------------------------- #

@pytest.mark.parametrize('mode,label,rows', [('valid', None, slice(2, 8)), ('valid', 'end', slice(2, 8)), ('valid', 'centre', slice(1, 7)),
                                             ('valid', 'start', slice(0, 6)), ('same', None, slice(0, 8)), ('same', 'centre', slice(0, 8))])
def test_time_filter(mode, label, rows):
    x = _field()
    out, cnt = V.time_filter(x, TAPS, mode=mode, label=label, return_count=True)
    _check(out, ('time', 'lat', 'lon'), {'time': TIMES[rows], 'lat': LAT}, 'time_filter', True)
    _check(cnt, ('time', 'lat', 'lon'), {'time': TIMES[rows], 'lat': LAT}, 'time_filter_count', True)


def test_windows():
    x = _field()
    out, cnt = V.running_mean(x, 3, step=2, return_count=True)
    _check(out, ('time', 'lat', 'lon'), {'time': TIMES[[2, 4, 6]], 'lat': LAT}, 'running_mean', True)
    _check(cnt, ('time', 'lat', 'lon'), {'time': TIMES[[2, 4, 6]], 'lat': LAT}, 'running_mean_count', True)
    # a filtered axis without a coordinate gets none
    _check(V.running_mean(x, 2, axis='lon'), ('time', 'lat', 'lon'), TL, 'running_mean', True)
    _check(V.lead_window_mean(x, [(0, 2), (2, 5)], axis='time'), ('time', 'lat', 'lon'), {'time': TIMES[[1, 4]], 'lat': LAT},
           'lead_window_mean', True)
    lead = Forecast(_array(), ('f_hour', 'lat', 'lon'), {'f_hour': np.arange(8) * 6}, name='x')
    _check(V.lead_window_mean(lead, [(0, 4), (4, 8)]), ('f_hour', 'lat', 'lon'), {'f_hour': np.array([18, 42])}, 'lead_window_mean', False)


def test_fits():
    x = _field()
    coef, cnt = V.time_regression(x, BASIS, return_count=True)
    _check(coef, ('term', 'lat', 'lon'), {'term': np.arange(2), 'lat': LAT}, 'time_regression', True)
    _check(cnt, ('lat', 'lon'), {'lat': LAT}, 'time_regression_count', True)
    mid = Forecast(np.moveaxis(x.values, 0, 1), ('lat', 'time', 'lon'), TL, name='x')
    _check(V.time_regression(mid, BASIS), ('lat', 'term', 'lon'), {'term': np.arange(2), 'lat': LAT}, 'time_regression', False)
    _check(V.regression_fitted(coef, BASIS[:5]), ('time', 'lat', 'lon'), {'lat': LAT}, 'regression_fitted', True)
    _check(V.regression_fitted(coef, BASIS[:5], times=TIMES[:5]), ('time', 'lat', 'lon'), {'time': TIMES[:5], 'lat': LAT},
           'regression_fitted', True)
    _check(V.regression_residual(x, coef, BASIS), ('time', 'lat', 'lon'), TL, 'regression_residual', True)
    _check(V.detrend(x), ('time', 'lat', 'lon'), TL, 'detrend', True)


def test_harmonic_climatology():
    x = _field()
    clim = V.harmonic_climatology(x, n_harmonics=1)
    _check(clim.coefficients, ('term', 'lat', 'lon'), {'term': np.arange(3), 'lat': LAT}, 'harmonic_climatology', True)
    _check(clim.series(TIMES[:3]), ('time', 'lat', 'lon'), {'time': TIMES[:3], 'lat': LAT}, 'climatology', True)
    _check(clim.series(TIMES[:3], f_hour=[0, 24]), ('f_hour', 'time', 'lat', 'lon'),
           {'f_hour': np.array([0, 24]), 'time': TIMES[:3], 'lat': LAT}, 'climatology', True)
    _check(clim.anomalies(x), ('time', 'lat', 'lon'), TL, 'anomaly', True)


def test_time_spectra():
    x, y = _field(), _field(1)
    f = np.arange(3) / 4.
    res, cnt = V.time_spectrum(x, 4, return_count=True)
    _check(res, ('frequency', 'lat', 'lon'), {'frequency': f, 'lat': LAT}, 'time_spectrum', True)
    _check(cnt, ('lat', 'lon'), {'lat': LAT}, 'time_spectrum_count', False)
    cross, cnt = V.time_cross_spectrum(x, y, 4, n_freq=2, return_count=True)
    for part, name in zip(cross, ('power_a', 'power_b', 'co', 'quad')):
        _check(part, ('frequency', 'lat', 'lon'), {'frequency': f[:2], 'lat': LAT}, name, True)
    _check(cnt, ('lat', 'lon'), {'lat': LAT}, 'time_cross_spectrum_count', False)
    res, cnt = V.time_coherence(x, y, 4, return_count=True)
    _check(res, ('frequency', 'lat', 'lon'), {'frequency': f, 'lat': LAT}, 'time_coherence', True)
    _check(cnt, ('lat', 'lon'), {'lat': LAT}, 'time_coherence_count', False)
    _check(V.time_spectrum(x, 4, axis='lon'), ('time', 'lat', 'frequency'), dict(TL, frequency=f), 'time_spectrum', True)
    _check(V.time_fourier(x), ('frequency', 'lat', 'lon'), {'frequency': np.arange(5) / 8., 'lat': LAT}, 'time_fourier', True)
    # the segment dim has no coordinate
    _check(V.time_fourier(x, n_segment=4), ('segment', 'frequency', 'lat', 'lon'), {'frequency': f, 'lat': LAT}, 'time_fourier', True)


def test_wavenumber_frequency():
    x = _field()
    f, k = np.arange(3) / 4., np.arange(4)
    res, cnt = V.wavenumber_frequency_spectrum(x, 4, return_count=True)
    for part, name in zip(res, ('eastward', 'westward')):
        _check(part, ('frequency', 'lat', 'wavenumber'), {'frequency': f, 'lat': LAT, 'wavenumber': k}, name, True)
    _check(cnt, ('lat', 'wavenumber'), {'lat': LAT, 'wavenumber': k}, 'wavenumber_frequency_spectrum_count', False)
    east, _ = V.wavenumber_frequency_spectrum(x, 4, n_wave=2, component='symmetric')
    _check(east, ('frequency', 'lat', 'wavenumber'), {'frequency': f, 'lat': LAT, 'wavenumber': k[:2]}, 'eastward', True)


# --------------------------------------------------------------------------------------------------------------------- #
# an unlabelled input comes back bare
# --------------------------------------------------------------------------------------------------------------------- #

def _ens_array():
    return np.stack([_array(s) for s in range(3)])


BARE = {
    'zonal_spectrum': lambda a: V.zonal_spectrum(a),
    'zonal_cross_spectrum': lambda a: V.zonal_cross_spectrum(a, a + 1.),
    'zonal_coherence': lambda a: V.zonal_coherence(a, a + 1.),
    'spherical_spectrum': lambda a: V.spherical_spectrum(a, lat=LAT),
    'spherical_cross_spectrum': lambda a: V.spherical_cross_spectrum(a, a + 1., lat=LAT),
    'spherical_correlation': lambda a: V.spherical_correlation(a, a + 1., lat=LAT),
    'spherical_analysis': lambda a: V.spherical_analysis(a, lat=LAT),
    'spherical_synthesis': lambda a: V.spherical_synthesis(V.spherical_analysis(a, lat=LAT), LAT, 6),
    'spherical_filter': lambda a: V.spherical_filter(a, lat=LAT),
    'spherical_laplacian': lambda a: V.spherical_laplacian(a, lat=LAT),
    'spherical_gradient': lambda a: V.spherical_gradient(a, lat=LAT),
    'spherical_vrtdiv': lambda a: V.spherical_vrtdiv(a, a + 1., lat=LAT),
    'spherical_uv': lambda a: V.spherical_uv(*V.spherical_vrtdiv(a, a + 1., lat=LAT), LAT, 6),
    'stack_forecasts': lambda a: V.stack_forecasts([a, a]),
    'ensemble_mean': lambda a: V.ensemble_mean(_ens_array()),
    'ensemble_spread': lambda a: V.ensemble_spread(_ens_array()),
    'ensemble_crps': lambda a: V.ensemble_crps(_ens_array(), a),
    'rank_histogram': lambda a: V.rank_histogram(_ens_array(), a, axis=(1, 2)),
    'ensemble_probability': lambda a: V.ensemble_probability(_ens_array(), [0.]),
    'brier_score': lambda a: V.brier_score(_ens_array(), a, [0.]),
    'ranked_probability_score': lambda a: V.ranked_probability_score(_ens_array(), a, [0.]),
    'reliability_counts': lambda a: V.reliability_counts(_ens_array(), a, [0.]),
    'time_filter': lambda a: V.time_filter(a, TAPS, return_count=True),
    'running_mean': lambda a: V.running_mean(a, 3),
    'lead_window_mean': lambda a: V.lead_window_mean(a, [(0, 2)]),
    'time_regression': lambda a: V.time_regression(a, BASIS, return_count=True),
    'regression_fitted': lambda a: V.regression_fitted(V.time_regression(a, BASIS), BASIS),
    'regression_residual': lambda a: V.regression_residual(a, V.time_regression(a, BASIS), BASIS),
    'detrend': lambda a: V.detrend(a),
    'time_spectrum': lambda a: V.time_spectrum(a, 4, return_count=True),
    'time_cross_spectrum': lambda a: V.time_cross_spectrum(a, a + 1., 4, return_count=True)[0],
    'time_coherence': lambda a: V.time_coherence(a, a + 1., 4),
    'time_fourier': lambda a: V.time_fourier(a, n_segment=4),
    'wavenumber_frequency_spectrum': lambda a: (lambda res, cnt: tuple(res) + (cnt,))(
        *V.wavenumber_frequency_spectrum(a, 4, return_count=True)),
}


@pytest.mark.parametrize('name', sorted(BARE))
def test_plain_array_in_plain_array_out(name):
    res = BARE[name](_array())
    for part in (tuple(res) if isinstance(res, tuple) else (res,)):
        assert type(part) is np.ndarray, type(part)


# --------------------------------------------------------------------------------------------------------------------- #
# axis resolution: every message
# --------------------------------------------------------------------------------------------------------------------- #

def _raises(kind, message, call):
    with pytest.raises(kind) as err:
        call()
    assert str(err.value) == message


def test_axis_position_out_of_range():
    a, e = _array(), _ens_array()
    _raises(ValueError, 'lon_axis 3 out of range of 3 axes', lambda: V.zonal_spectrum(a, lon_axis=3))
    _raises(ValueError, 'lon_axis -4 out of range of 3 axes', lambda: V.wavenumber_frequency_spectrum(a, 4, lon_axis=-4))
    _raises(ValueError, 'lat_axis 5 out of range of 3 axes', lambda: V.spherical_spectrum(a, lat=LAT, lat_axis=5))
    _raises(ValueError, 'lon_axis -4 out of range of 3 axes', lambda: V.spherical_filter(a, lat=LAT, lon_axis=-4))
    _raises(ValueError, 'member_axis 4 out of range of 4 axes', lambda: V.ensemble_mean(e, member_axis=4))
    _raises(ValueError, 'member_axis -5 out of range of 4 axes', lambda: V.brier_score(e, a, [0.], member_axis=-5))
    _raises(ValueError, 'threshold_axis 4 out of range of 4 axes',
            lambda: V.ensemble_probability(e, np.zeros((2, 8, 4, 6)), threshold_axis=4))
    _raises(ValueError, 'axis 3 is out of range of 3 dims', lambda: V.time_filter(a, TAPS, axis=3))
    _raises(ValueError, 'axis -4 is out of range of 3 dims', lambda: V.time_regression(a, BASIS, axis=-4))
    _raises(ValueError, 'axis 3 is out of range of 3 dims', lambda: V.time_spectrum(a, 4, axis=3))
    _raises(ValueError, 'axis 3 is out of range of 3 dims', lambda: V.regression_fitted(V.time_regression(a, BASIS), BASIS, term_axis=3))


def test_axis_by_name():
    x = _field()
    _raises(ValueError, "the ensemble's dims ('time', 'lat', 'lon') have no 'member'", lambda: V.ensemble_mean(x))
    _raises(ValueError, "the ensemble's dims ('time', 'lat', 'lon') have no 'member'", lambda: V.reliability_counts(x, x, [0.]))
    for call in (lambda: V.time_filter(x, TAPS, axis='level'), lambda: V.lead_window_mean(x, [(0, 2)], axis='level'),
                 lambda: V.detrend(x, axis='level'), lambda: V.time_fourier(x, axis='level')):
        _raises(ValueError, "the data has no 'level' dimension (dims: time, lat, lon)", call)
    _raises(ValueError, "the data has no 'time' dimension (dims: )", lambda: V.running_mean(_array(), 3, axis='time'))
    # a name among the averaged axes is looked up with tuple.index
    _raises(ValueError, 'tuple.index(x): x not in tuple', lambda: V.zonal_spectrum(x, axis='level'))
    _raises(ValueError, 'tuple.index(x): x not in tuple', lambda: V.spherical_spectrum(x, axis=('time', 'level')))
    # a labelled input's own dims win over the positions given; an explicit `axis` wins over the 'time' dim
    swapped = Forecast(np.moveaxis(_array(), 2, 0), ('lon', 'time', 'lat'), TL, name='x')
    _check(V.zonal_spectrum(swapped, lon_axis=-1, axis='time'), ('lat', 'wavenumber'), {'lat': LAT, 'wavenumber': np.arange(4)},
           'zonal_spectrum', False)
    _check(V.spherical_spectrum(swapped, lat_axis=0, lon_axis=1), ('degree',), {'degree': np.arange(2)}, 'spherical_spectrum', False)
    _check(V.running_mean(swapped, 2, axis=2), ('lon', 'time', 'lat'), {'time': TIMES, 'lat': LAT[1:]}, 'running_mean', False)
    # a labelled input without the dim looked for falls back to the position
    nameless = Forecast(_array(), ('time', 'y', 'x'), {'time': TIMES}, name='x')
    _check(V.zonal_spectrum(nameless, axis=0), ('y', 'wavenumber'), {'wavenumber': np.arange(4)}, 'zonal_spectrum', False)
    _check(V.running_mean(Forecast(_array(), ('f_hour', 'y', 'x'), {}, name='x'), 2), ('f_hour', 'y', 'x'), {}, 'running_mean', False)


def test_transformed_axis_cannot_be_averaged():
    x = _field()
    _raises(ValueError, 'the longitude axis is transformed, it cannot be averaged over', lambda: V.zonal_spectrum(x, axis='lon'))
    _raises(ValueError, 'the longitude axis is transformed, it cannot be averaged over', lambda: V.zonal_coherence(_array(), _array(1), axis=(0, -1)))
    _raises(ValueError, 'the latitude and longitude axes are transformed, they cannot be averaged over',
            lambda: V.spherical_spectrum(x, axis='lat'))
    _raises(ValueError, 'the latitude and longitude axes are transformed, they cannot be averaged over',
            lambda: V.spherical_correlation(_array(), _array(1), lat=LAT, axis=2))


def test_first_import_of_labelled_is_light():
    """the labelled-array layer is a leaf: importing it brings in neither torch nor the model package"""
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'dlwp-cs_amd')
    code = ('import sys; sys.path.insert(0, %r); import DLWP.labelled; '
            'bad = [m for m in ("torch", "DLWP.model") if m in sys.modules]; assert not bad, bad' % pkg)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_forecast_has_one_home():
    import DLWP.labelled
    import DLWP.model
    import DLWP.model.extensions
    assert DLWP.model.extensions.Forecast is DLWP.labelled.Forecast is V.Forecast
