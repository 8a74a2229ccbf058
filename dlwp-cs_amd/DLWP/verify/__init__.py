"""
Scoring forecasts (reference DLWP/verify.py:18-164: `forecast_error`, `persistence_error`, `climo_error`) and labelling a
cubed-sphere forecast array (behaviour of reference DLWP/verify.py:291-325, pinned by tests/golden/g11_verify.npz:
dimension names and order, coordinate values, the split of the channel axis into variable x level).

Climatologies (reference DLWP/verify.py:167-214, 426-456: `monthly_climo_error`, `daily_climatology`,
`daily_climo_time_series`): grouped means over the time axis by month or day of the year, on the device where the values lie.
`climatology_quantiles` gives grouped quantiles the same way (tercile boundaries), and `ensemble_probability`, `brier_score`,
`ranked_probability_score`, `categorical_error` and `reliability_counts` score an ensemble against them; the reference has no
counterpart of these.

The engine has no xarray: the labelled result is the `Forecast` record of DLWP.labelled (values, dimension names, one
coordinate array per dimension, `isel`), and every family reads its inputs, finds its axes and labels its results through that
module.  `meta_ds` is anything with a `dims` mapping {name: size} and `meta_ds[name]` -> coordinate values -- an xarray.Dataset
qualifies.

One module per family, each importing only from DLWP.labelled and from the modules before it: scores, climatology, zonal,
spherical, ensemble, category, timeseries, eof, resample, spells, ranks.  This file is the public face and holds imports only.

The scores take the reference's arguments and give its result shapes, warnings and errors (INTEGRATION.md lists where the
engine differs: the cases the reference cannot run).  Inputs that live on a HIP device -- torch tensors, or a `Forecast` whose
values are one -- are scored by the dlwpcs_score kernel where they lie and only the score table is downloaded; numpy inputs are
scored on the host by a numpy restatement of the same formulas.  Results are float64 numpy arrays.
"""
# public names first, then the private ones that tests and tools reach through the package
from ..labelled import Forecast, axes as _axes  # noqa: F401
from .scores import (add_metadata_to_forecast_cs, climo_error, forecast_error, persistence_error, _nanmean,  # noqa: F401
                     _score_host, _weights)
from .climatology import (calendar_keys, climatology_quantiles, ClimatologyLookup, daily_climatology,  # noqa: F401
                          daily_climo_time_series, monthly_climo_error, _csr, _group_quantile_host)
from .zonal import CrossSpectrum, zonal_coherence, zonal_cross_spectrum, zonal_spectrum  # noqa: F401
from .spherical import (spherical_analysis, spherical_correlation, spherical_cross_spectrum, spherical_filter,  # noqa: F401
                        spherical_gradient, spherical_laplacian, spherical_spectrum, spherical_synthesis,
                        spherical_uv, spherical_vrtdiv, SphericalCrossSpectrum)
from .ensemble import (ensemble_crps, ensemble_error, ensemble_mean, ensemble_spread, rank_histogram,  # noqa: F401
                       stack_forecasts, _ENS_METHODS, _ensemble_fields)
from .category import (brier_score, categorical_error, ensemble_probability, ranked_probability_score,  # noqa: F401
                       reliability_counts, _CAT_METHODS, _category_fields)
from .timeseries import (autocorrelation, decorrelation_time, detrend, effective_sample_size, harmonic_basis,  # noqa: F401
                         harmonic_climatology, HarmonicClimatology, lag_correlation, lag_covariance, lag_regression,
                         lanczos_weights, lead_window_mean, regression_fitted, REGRESSION_MAX_TERMS, regression_residual,
                         running_mean, spectral_window, time_coherence, time_cross_spectrum, time_filter,
                         time_fourier, time_regression, time_spectrum, TimeCrossSpectrum,
                         wavenumber_frequency_spectrum, WavenumberFrequencySpectrum, _time_lag_host)
from .eof import eof_analysis, EOFAnalysis, EOF_MAX_ROWS, pattern_covariance, _gram_host  # noqa: F401
from .resample import (bootstrap_difference, bootstrap_interval, bootstrap_mean, bootstrap_starts, BootstrapInterval,  # noqa: F401
                       _resample_host)
from .spells import (spell_length, spell_mask, spell_position, spell_statistics, SpellStatistics, _spell_host)  # noqa: F401
from .ranks import (kendall_tau, KendallTau, mann_kendall, MannKendall, spearman_correlation, time_ranks,  # noqa: F401
                    _rank_host)
