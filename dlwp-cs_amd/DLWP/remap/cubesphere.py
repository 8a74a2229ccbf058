"""
Remapping between the cubed sphere and a lat-lon grid with existing offline maps (reference DLWP/remap/cubesphere.py).

The reference drives TempestRemap's executables on netCDF files.  Here the maps are read once (DLWP.remap.read_offline_map)
and applied to arrays: device tensors by the dlwpcs_sparse_map_apply kernel where they lie, numpy arrays on the host.  The
file-to-file methods need TempestRemap or xarray, which this stack does not have; they raise NotImplementedError.
"""
import os
import sys

from ..model.extensions import Forecast
from .offline_map import OfflineMap, read_offline_map

_CUBE_DIMS = (('x0', 'x1', 'x2'), ('face', 'height', 'width'))
_FILE_MSG = ('CubeSphereRemap.%s needs the TempestRemap executables or xarray, which this engine does not use; apply an '
             'existing offline map to arrays with remap_array / inverse_remap_array / inverse_remap_forecast instead')


class CubeSphereRemap(object):
    """
    Remap arrays to and from a cubed sphere with offline maps (the reference's CubeSphereRemap, array methods only).

    :param path_to_remapper: kept for the reference's signature (the TempestRemap executables are not run)
    :param to_netcdf4: kept for the reference's signature (maps are read from netCDF classic / 64-bit-offset files)
    :param verbose: print a line when a map file is loaded
    """

    def __init__(self, path_to_remapper=None, to_netcdf4=True, verbose=True):
        self.path_to_remapper = os.path.dirname(sys.executable) if path_to_remapper is None else path_to_remapper
        self.remapper = os.path.join(self.path_to_remapper, 'ApplyOfflineMap')
        self.map = None
        self.inverse_map = None
        self.to_netcdf4 = to_netcdf4
        self.verbose = verbose
        self._lat = None
        self._lon = None
        self._res = None
        self._map_exists = False
        self._inverse_map_exists = False
        self._loaded = {}

    def assign_maps(self, map_name=None, inverse_map_name=None):
        """
        Point to either or both of the forward (lat-lon -> cube) and inverse (cube -> lat-lon) maps: file paths, read at
        first use, or OfflineMap objects.

        :param map_name: str or OfflineMap: forward map
        :param inverse_map_name: str or OfflineMap: inverse map
        """
        if map_name is not None:
            self.map = map_name
            self._map_exists = True
            self._loaded.pop('forward', None)
        if inverse_map_name is not None:
            self.inverse_map = inverse_map_name
            self._inverse_map_exists = True
            self._loaded.pop('inverse', None)

    def _get(self, which):
        hit = self._loaded.get(which)
        if hit is not None:
            return hit
        src, exists = (self.map, self._map_exists) if which == 'forward' else (self.inverse_map, self._inverse_map_exists)
        if not exists:
            raise ValueError("No %s map has been defined; use the 'assign_maps' function first" % which)
        if isinstance(src, OfflineMap):
            m = src
        else:
            if not os.path.exists(src):
                raise FileNotFoundError(src)
            m = read_offline_map(src)
            if self.verbose:
                print('CubeSphereRemap: loaded %s map %s' % (which, m))
        self._loaded[which] = m
        return m

    def remap_array(self, x, axes=(-2, -1)):
        """
        Lat-lon -> cubed sphere with the forward map: the (lat, lon) axes of x are replaced in place by (face, height, width).
        numpy input: host path, the input's float dtype.  HIP tensor (fp32 or bf16): fp32 device result, one launch.
        """
        return self._get('forward').apply(x, axes)

    def inverse_remap_array(self, x, axes=(-3, -2, -1)):
        """
        Cubed sphere -> lat-lon with the inverse map: the (face, height, width) axes of x are replaced by (lat, lon).
        numpy input: host path, the input's float dtype.  HIP tensor (fp32 or bf16): fp32 device result, one launch.
        """
        return self._get('inverse').apply(x, axes)

    def inverse_remap_forecast(self, forecast):
        """
        Inverse-remap a labelled cubed-sphere forecast (a Forecast whose space dims are 'x0', 'x1', 'x2' as from
        TimeSeriesEstimator.predict / verification, or 'face', 'height', 'width' as from add_metadata_to_forecast_cs).
        Returns a Forecast with 'lat', 'lon' in their place and the map's coordinates; the values stay on the device when they
        came from there.  `.lat` / `.lon` are Forecasts of dims ('lat',) / ('lon',), so forecast_error(..., weighted=True)
        weights by latitude.  NaN cells (a verification past the end of the data) propagate to every row they feed.
        """
        dims = tuple(forecast.dims)
        a0 = None
        for names in _CUBE_DIMS:
            for i in range(len(dims) - 2):
                if dims[i:i + 3] == names:
                    a0 = i
        if a0 is None:
            raise ValueError("forecast dims %s have none of ('x0', 'x1', 'x2') / ('face', 'height', 'width')" % (dims,))
        m = self._get('inverse')
        if m.dst_kind != 'latlon' or m.lat_b is None:
            raise ValueError('the inverse map %s has no lat-lon destination with cell centres (yc_b / xc_b)' % m)
        vals = m.apply(forecast.values, (a0, a0 + 1, a0 + 2))
        new_dims = dims[:a0] + ('lat', 'lon') + dims[a0 + 3:]
        coords = {d: c for d, c in forecast.coords.items() if d in new_dims}
        coords['lat'], coords['lon'] = m.lat_b.copy(), m.lon_b.copy()
        out = Forecast(vals, new_dims, coords, name=forecast.name)
        out.lat = Forecast(coords['lat'], ('lat',), {'lat': coords['lat']}, name='lat')
        out.lon = Forecast(coords['lon'], ('lon',), {'lon': coords['lon']}, name='lon')
        return out

    # file-to-file methods of the reference: TempestRemap executables / xarray
    def generate_offline_maps(self, *args, **kwargs):
        raise NotImplementedError(_FILE_MSG % 'generate_offline_maps')

    def generate_offline_maps_from_file(self, *args, **kwargs):
        raise NotImplementedError(_FILE_MSG % 'generate_offline_maps_from_file')

    def remap(self, *args, **kwargs):
        raise NotImplementedError(_FILE_MSG % 'remap')

    def inverse_remap(self, *args, **kwargs):
        raise NotImplementedError(_FILE_MSG % 'inverse_remap')

    def convert_to_faces(self, *args, **kwargs):
        raise NotImplementedError(_FILE_MSG % 'convert_to_faces')

    def convert_from_faces(self, *args, **kwargs):
        raise NotImplementedError(_FILE_MSG % 'convert_from_faces')
