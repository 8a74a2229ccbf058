#
# Utilities of the MI355X-native DLWP-CS engine (subset of the reference's DLWP/util.py that the hot path touches).
#

"""
Model persistence and small helpers.  `save_model` / `load_model` keep the reference's file triple
(`<name>.keras` model, `<name>.pkl` wrapper, `<name>.history`; reference DLWP/util.py:127-193); the `.keras` file is
written in the engine's native format (pickled config + numpy weights) because HDF5 needs h5py + TensorFlow.
"""

import importlib
import pickle
import re
from copy import copy

import numpy as np


def make_keras_picklable():
    """No-op: DLWP.keras models are plain Python objects (the reference patched keras.Model, util.py:28-80)."""
    return None


def get_from_class(module_name, class_name):
    """Return `class_name` from module `module_name` (reference DLWP/util.py:83-94)."""
    mod = importlib.import_module(module_name)
    return getattr(mod, class_name)


def get_classes(module_name):
    """dict name -> class for every class of a module (reference DLWP/util.py:97-110)."""
    mod = importlib.import_module(module_name)
    return {k: getattr(mod, k) for k in dir(mod) if isinstance(getattr(mod, k), type)}


def get_methods(module_name):
    """dict name -> callable for every callable of a module (reference DLWP/util.py:113-124)."""
    mod = importlib.import_module(module_name)
    return {k: getattr(mod, k) for k in dir(mod) if callable(getattr(mod, k))}


def save_model(model, file_name, history=None):
    """
    Save a DLWP wrapper (an object with a `model` attribute): `<file_name>.keras` (model + weights + optimizer state),
    `<file_name>.pkl` (the wrapper without the model) and, if given, `<file_name>.history`.
    """
    net = model.base_model if hasattr(model, 'base_model') else model.model
    net.save('%s.keras' % file_name)
    model_copy = copy(model)
    model_copy.model = None
    if hasattr(model, 'base_model'):
        model_copy.base_model = None
    with open('%s.pkl' % file_name, 'wb') as f:
        pickle.dump(model_copy, f, protocol=pickle.HIGHEST_PROTOCOL)
    if history is not None:
        with open('%s.history' % file_name, 'wb') as f:
            pickle.dump(history.history, f, protocol=pickle.HIGHEST_PROTOCOL)


def load_model(file_name, history=False, custom_objects=None, gpus=1):
    """
    Load a model saved with `save_model`.  Every class of DLWP.custom is available to the loader automatically.

    :return: model [, history dict]
    """
    from .keras import models as keras_models
    with open('%s.pkl' % file_name, 'rb') as f:
        model = pickle.load(f)
    custom_objects = dict(custom_objects or {})
    custom_objects.update(get_classes('DLWP.custom'))
    loaded = keras_models.load_model('%s.keras' % file_name, custom_objects=custom_objects, compile=True)
    model.base_model = loaded
    model.model = loaded
    if gpus > 1:
        model.gpus = gpus
    if history:
        with open('%s.history' % file_name, 'rb') as f:
            h = pickle.load(f)
        return model, h
    return model


def to_bool(v):
    """Parse a command-line style boolean (reference DLWP/util.py:385-401)."""
    if isinstance(v, bool):
        return v
    if str(v).lower() in ('yes', 'true', 't', 'y', '1'):
        return True
    if str(v).lower() in ('no', 'false', 'f', 'n', '0'):
        return False
    raise ValueError('Boolean value expected.')


def remove_chars(s):
    """Strip characters with unintended effects on file paths (reference DLWP/util.py:425-431)."""
    return ''.join(re.split('[$/\\\\]', s))


def is_channels_last(model):
    """True if the first layer that has a `data_format` uses channels_last (reference DLWP/util.py:434-444)."""
    for layer in model.model.layers:
        if hasattr(layer, 'data_format'):
            return layer.data_format == 'channels_last'
    return False


def _solar_grid(lat, lon):
    """(lat, lon) of `insolation` as arrays of one shape: two 1-d axes form a regular grid."""
    lat, lon = np.asarray(lat), np.asarray(lon)
    if lat.ndim != lon.ndim:
        raise ValueError("'lat' and 'lon' must either both be 1d or both be 2d'")
    if lat.ndim >= 2 and lat.shape != lon.shape:
        raise ValueError("shape mismatch between lat (%s) and lon (%s)" % (lat.shape, lon.shape))
    if lat.ndim == 1:
        lon, lat = np.meshgrid(lon, lat)
    return lat, lon


def _solar_day(dates, daily=False):
    """fractional day of the year (leap days ignored) of every date, float32 like the reference: the hour angle inherits its
    rounding.  daily: the local noon of the day."""
    import pandas as pd
    stamps = pd.DatetimeIndex(pd.to_datetime(list(dates)))
    start = pd.DatetimeIndex([pd.Timestamp(d.year, 1, 1) for d in stamps])
    day = ((stamps - start).total_seconds() / 86400.).values.astype(np.float32)
    if daily:
        day = 0.5 + np.round(day)
    return day


def _solar_orbit(day):
    """(declination, sun-earth distance) at `day`, elementwise; orbital constants of 1995"""
    obliquity, ecc, perihelion = np.deg2rad(23.4441), 0.016715, np.deg2rad(282.7)
    mean_lon = ecc * (1. + np.sqrt(1 - ecc ** 2.)) * np.sin(perihelion) + 2. * np.pi * (day - 80.5) / 365.
    true_lon = mean_lon + 2. * ecc * np.sin(mean_lon - perihelion)
    decl = np.arcsin(np.sin(obliquity) * np.sin(true_lon))
    dist = (1. - ecc ** 2.) / (1. + ecc * np.cos(true_lon - perihelion))
    return decl, dist


def insolation(dates, lat, lon, S=1., daily=False, device=None):
    """
    Approximate top-of-atmosphere solar insolation, the `solar` input channel of the DLWP-CS models (reference
    DLWP/util.py:306-364; pinned to the reference by tests/golden/g6_insolation.npz).

    :param dates: 1-d sequence of datetimes / Timestamps / datetime64
    :param lat, lon: both 1-d (a regular grid is formed) or both N-d of equal shape (e.g. cubed-sphere (6, N, N)); degrees,
        lon in 0-360
    :param S: solar constant scaling
    :param daily: True -> daily maximum (local noon) instead of the instantaneous value
    :param device: None -> computed on the host; a torch device / True (the engine's device) -> computed on the device by
        `dlwpcs_solar_fill` from the tables of a `SolarForcing` (differs from the host result through the cosine only)
    :return: float32 array (date, *grid); with `device`, a float32 device tensor of that shape
    """
    if device is not None and device is not False:
        return SolarForcing(dates, lat, lon, S=S, daily=daily).to_device(device)
    lat, lon = _solar_grid(lat, lon)
    day = _solar_day(dates, daily)
    day = day.reshape((-1,) + (1,) * lat.ndim)
    lon32 = lon.astype(np.float32)
    if daily:
        lon32 = np.zeros_like(lon32)
    decl, dist = _solar_orbit(day)
    hour = 2 * np.pi * (day + lon32 / 360.)
    phi = np.deg2rad(lat)[None, ...]
    sol = S * (np.sin(phi) * np.sin(decl) - np.cos(phi) * np.cos(decl) * np.cos(hour)) * dist ** -2.
    return np.maximum(sol, 0.).astype(np.float32)


class SolarForcing(object):
    """
    The insolation field of `insolation(dates, lat, lon, S, daily)` described instead of stored: a lazy (T, *grid) float32
    "array" that is accepted wherever an `insolation_array` is.

      * On the host, rows are evaluated on demand through `insolation` (`sf[rows]`, `np.asarray(sf)`): bitwise the dense array.
      * On the device nothing of size T x cells exists: `tables(device)` uploads a row table (T, 4) = {sin(decl), cos(decl),
        S * dist**-2, day} and a cell table (cells, 3) = {sin(phi), cos(phi), lon / 360} (float64, built here with the numpy
        expressions and dtypes of `insolation`), and `DLWP.ops.solar_fill` computes every value where it is written.
      * `rows(n)` continues the record past `dates` in steps of `dt`, so a forecast can run beyond the end of the data.
    """

    ROW_CHUNK = 64                      # rows(n) grows in chunks: a series of forecasts shares one table (and one captured graph)

    def __init__(self, dates, lat, lon, S=1., daily=False, dt=None):
        import pandas as pd
        self.dates = pd.DatetimeIndex(pd.to_datetime(list(dates)))
        self.lat, self.lon = _solar_grid(lat, lon)
        self.S, self.daily = S, bool(daily)
        if dt is None and len(self.dates) > 1:
            dt = self.dates[1] - self.dates[0]
        self.dt = None if dt is None else pd.Timedelta(dt)
        day = _solar_day(self.dates, self.daily)
        decl, dist = _solar_orbit(day)
        #: (T, 4) float64: sin(decl), cos(decl), S * dist**-2, day (float32 values)
        self.row_table = np.stack([np.sin(decl), np.cos(decl), S * dist ** -2., day], axis=1).astype(np.float64)
        lon32 = self.lon.astype(np.float32)
        if self.daily:
            lon32 = np.zeros_like(lon32)
        phi = np.deg2rad(self.lat)
        #: (cells, 3) float64: sin(phi), cos(phi), lon / 360 (float32 values)
        self.cell_table = np.stack([np.sin(phi).reshape(-1), np.cos(phi).reshape(-1), (lon32 / 360.).reshape(-1)],
                                   axis=1).astype(np.float64)
        self._dev = {}
        self._longer = None

    def __getstate__(self):
        state = dict(self.__dict__)
        state['_dev'], state['_longer'] = {}, None
        return state

    @property
    def shape(self):
        return (len(self.dates),) + tuple(self.lat.shape)

    @property
    def ndim(self):
        return 1 + self.lat.ndim

    @property
    def dtype(self):
        return np.dtype(np.float32)

    @property
    def nbytes(self):
        """bytes of the two tables: what the device keeps resident"""
        return int(self.row_table.nbytes + self.cell_table.nbytes)

    def __len__(self):
        return len(self.dates)

    def __getitem__(self, key):
        rest = ()
        if isinstance(key, tuple):
            key, rest = key[0], tuple(key[1:])
        idx = np.arange(len(self))[key]                         # numpy's own index rules (and its IndexError)
        flat = np.atleast_1d(idx).reshape(-1)
        if flat.size:
            out = insolation(self.dates[flat], self.lat, self.lon, S=self.S, daily=self.daily)
        else:
            out = np.zeros((0,) + tuple(self.lat.shape), dtype=np.float32)
        out = out.reshape(np.shape(idx) + tuple(self.lat.shape))
        return out[(slice(None),) * np.ndim(idx) + rest] if rest else out

    def __array__(self, dtype=None, copy=None):
        out = insolation(self.dates, self.lat, self.lon, S=self.S, daily=self.daily)
        return out if dtype is None else out.astype(dtype, copy=False)

    def rows(self, n_rows):
        """
        A SolarForcing of at least `n_rows` rows: this one, or its continuation, whose rows past the last date follow it in steps
        of `dt` (for an evenly spaced record, row k at dates[0] + k * dt).  Only the added rows are evaluated; the cell table and
        the rows of this record are shared.  The continuation grows in chunks of ROW_CHUNK rows and the longest one is kept: it
        serves every shorter request.
        """
        n_rows = int(n_rows)
        if n_rows <= len(self):
            return self
        if self._longer is not None and len(self._longer) >= n_rows:
            return self._longer
        if self.dt is None or not len(self):
            raise IndexError('SolarForcing: %d rows wanted, %d dates and no time step to continue them' % (n_rows, len(self)))
        n_rows = -(-n_rows // self.ROW_CHUNK) * self.ROW_CHUNK
        base = self if self._longer is None else self._longer
        more = [base.dates[-1] + k * self.dt for k in range(1, n_rows - len(base) + 1)]
        longer = SolarForcing(more, self.lat, self.lon, S=self.S, daily=self.daily, dt=self.dt)
        longer.dates = base.dates.append(longer.dates)
        longer.row_table = np.concatenate([base.row_table, longer.row_table], axis=0)
        longer.cell_table = self.cell_table
        self._longer = longer
        return longer

    def tables(self, device):
        """(row table, cell table) as float64 tensors on `device`, uploaded once per device"""
        import torch
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.row_table).to(device), torch.from_numpy(self.cell_table).to(device))
        return self._dev[key]

    def to_device(self, device=True):
        """The dense (T, *grid) float32 tensor on `device` (True: the engine's device), written by the kernel."""
        import torch
        from . import ops
        from .keras import backend
        dev = backend.device() if device is True else torch.device(device)
        row, cell = self.tables(dev)
        out = torch.empty(self.shape, dtype=torch.float32, device=dev)
        if out.numel():
            ops.solar_fill(row, cell, torch.arange(len(self), dtype=torch.int32, device=dev), out.view(self.shape + (1,)),
                           1, 0, 1, 0, 1, True)
        return out
