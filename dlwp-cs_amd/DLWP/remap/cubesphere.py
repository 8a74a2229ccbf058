"""
Remapping between the cubed sphere and a lat-lon grid with existing offline maps (reference DLWP/remap/cubesphere.py).

The reference drives TempestRemap's executables on netCDF files.  Here the maps are read once (DLWP.remap.read_offline_map)
and applied to arrays: device tensors by the dlwpcs_sparse_map_apply kernel where they lie, numpy arrays on the host.  Maps
that do not exist yet are made by `generate_maps` (closed-form conservative maps, DLWP.remap.overlap).  Smooth output on a fine
lat-lon grid and values at a list of points come from `generate_sampling_map` (bilinear, DLWP.remap.bilinear).  The file-to-file
methods need TempestRemap or xarray, which this stack does not have; they raise NotImplementedError.
"""
import os
import sys

from ..model.extensions import Forecast
from .grid import CubeSphereGrid, LatLonGrid
from .offline_map import OfflineMap, read_offline_map, write_offline_map
from .overlap import conservative_maps
from .bilinear import bilinear_map

_CUBE_DIMS = (('x0', 'x1', 'x2'), ('face', 'height', 'width'))
_FILE_MSG = ('CubeSphereRemap.%s needs the TempestRemap executables or xarray, which this engine does not use; apply an '
             'existing offline map to arrays with remap_array / inverse_remap_array / inverse_remap_forecast instead')


def _missing_kw(kw, frac=True):
    """the missing-value keywords of OfflineMap.apply that the array / forecast methods hand through"""
    known = ('skipna', 'min_valid', 'renormalize') + (('frac_out',) if frac else ())
    for k in kw:
        if k not in known:
            raise TypeError('unexpected keyword %r (missing-value keywords: %s)' % (k, ', '.join(known)))
    return kw


def _cube_axis(dims):
    """first of the three consecutive cube dims of a labelled forecast"""
    dims, a0 = tuple(dims), None
    for names in _CUBE_DIMS:
        for i in range(len(dims) - 2):
            if dims[i:i + 3] == names:
                a0 = i
    if a0 is None:
        raise ValueError("forecast dims %s have none of ('x0', 'x1', 'x2') / ('face', 'height', 'width')" % (dims,))
    return a0


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
        self.cube_grid = None
        self.latlon_grid = None
        self.sampling_map = None

    def generate_maps(self, lat=None, lon=None, res=None, inverse_lat=False, lon_begin=0., *, grid=None, latlon=None,
                      device=None, map_name=None, inverse_map_name=None):
        """
        Make the forward (lat-lon -> cube) and inverse (cube -> lat-lon) first-order conservative maps and assign them, so that
        remap_array / inverse_remap_array / inverse_remap_forecast work at once.  The grids are kept as `.cube_grid` and
        `.latlon_grid` (cell centres for SolarForcing / TimeSeriesEstimator, cell areas).

        :param lat, lon: int: number of cells in latitude and longitude (as GenerateRLLMesh --lat --lon)
        :param res: int: number of cells on a side of each cube face
        :param inverse_lat: the latitudes of the data descend from 90
        :param lon_begin: the first longitude edge in degrees
        :param grid: CubeSphereGrid in place of `res` (e.g. CubeSphereGrid.from_centres of an existing data set)
        :param latlon: LatLonGrid in place of `lat`, `lon`, `inverse_lat` and `lon_begin`
        :param device: a HIP device: the overlap areas are computed by the dlwpcs_overlap_* kernels; None: on the host
        :param map_name, inverse_map_name: str: also write the map to this file (64-bit-offset netCDF, SCRIP layout)
        :return: (forward, inverse) OfflineMap
        """
        if latlon is None:
            if lat is None or lon is None:
                raise ValueError('generate_maps needs lat and lon, or latlon=')
            latlon = LatLonGrid.cells(int(lat), int(lon), inverse_lat=inverse_lat, lon_begin=lon_begin)
        elif not isinstance(latlon, LatLonGrid):
            raise TypeError('latlon must be a DLWP.remap.LatLonGrid')
        if grid is None:
            if res is None:
                raise ValueError('generate_maps needs res, or grid=')
            grid = CubeSphereGrid(int(res))
        elif not isinstance(grid, CubeSphereGrid):
            raise TypeError('grid must be a DLWP.remap.CubeSphereGrid')
        forward, inverse = conservative_maps(grid, latlon, device=device)
        forward.name = 'map_LL%dx%d_CS%d' % (latlon.n_lat, latlon.n_lon, grid.N)
        inverse.name = 'map_CS%d_LL%dx%d' % (grid.N, latlon.n_lat, latlon.n_lon)
        self._lat, self._lon, self._res = latlon.n_lat, latlon.n_lon, grid.N
        self.cube_grid, self.latlon_grid = grid, latlon
        if map_name is not None:
            write_offline_map(forward, map_name)
        if inverse_map_name is not None:
            write_offline_map(inverse, inverse_map_name)
        self.assign_maps(forward, inverse)
        return forward, inverse

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

    def remap_array(self, x, axes=(-2, -1), **missing):
        """
        Lat-lon -> cubed sphere with the forward map: the (lat, lon) axes of x are replaced in place by (face, height, width).
        numpy input: host path, the input's float dtype.  HIP tensor (fp32 or bf16): fp32 device result, one launch.
        skipna, min_valid, renormalize, frac_out: NaN cells are missing values, left out of the sums (OfflineMap.apply).
        """
        return self._get('forward').apply(x, axes, **_missing_kw(missing))

    def inverse_remap_array(self, x, axes=(-3, -2, -1), **missing):
        """
        Cubed sphere -> lat-lon with the inverse map: the (face, height, width) axes of x are replaced by (lat, lon).
        numpy input: host path, the input's float dtype.  HIP tensor (fp32 or bf16): fp32 device result, one launch.
        skipna, min_valid, renormalize, frac_out: NaN cells are missing values, left out of the sums (OfflineMap.apply).
        """
        return self._get('inverse').apply(x, axes, **_missing_kw(missing))

    def inverse_remap_forecast(self, forecast, **missing):
        """
        Inverse-remap a labelled cubed-sphere forecast (a Forecast whose space dims are 'x0', 'x1', 'x2' as from
        TimeSeriesEstimator.predict / verification, or 'face', 'height', 'width' as from add_metadata_to_forecast_cs).
        Returns a Forecast with 'lat', 'lon' in their place and the map's coordinates; the values stay on the device when they
        came from there.  `.lat` / `.lon` are Forecasts of dims ('lat',) / ('lon',), so forecast_error(..., weighted=True)
        weights by latitude.  NaN cells (a verification past the end of the data) propagate to every row they feed, unless
        skipna=True (with min_valid, renormalize as in OfflineMap.apply) leaves them out of the sums.
        """
        missing = _missing_kw(missing, frac=False)
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
        vals = m.apply(forecast.values, (a0, a0 + 1, a0 + 2), **missing)
        new_dims = dims[:a0] + ('lat', 'lon') + dims[a0 + 3:]
        coords = {d: c for d, c in forecast.coords.items() if d in new_dims}
        coords['lat'], coords['lon'] = m.lat_b.copy(), m.lon_b.copy()
        out = Forecast(vals, new_dims, coords, name=forecast.name)
        out.lat = Forecast(coords['lat'], ('lat',), {'lat': coords['lat']}, name='lat')
        out.lon = Forecast(coords['lon'], ('lon',), {'lon': coords['lon']}, name='lon')
        return out

    # ---------------------------------------------------------------------------------------------------------------- #
    # bilinear sampling of the cube: smooth lat-lon output, values at points
    def generate_sampling_map(self, lat=None, lon=None, *, latlon=None, grid=None, res=None, device=None, map_name=None):
        """
        Make the bilinear sampling map from the cube (DLWP.remap.bilinear: continuous across face edges and corners) and keep
        it as `.sampling_map` for sample_array / sample_forecast.  The conservative maps are not touched.

        :param lat, lon: arrays of one shape: the points to sample at, in degrees (any finite longitude)
        :param latlon: LatLonGrid in place of the points: its cell centres are sampled and the result has (lat, lon) axes
        :param grid: CubeSphereGrid; or `res`: cells on a side of each cube face; default: the grid of generate_maps
        :param device: a HIP device: the weights are computed by the dlwpcs_cube_bilinear kernel; None: on the host
        :param map_name: str: also write the map to this file (64-bit-offset netCDF, SCRIP layout)
        :return: OfflineMap
        """
        if grid is None:
            if res is not None:
                grid = CubeSphereGrid(int(res))
            elif self.cube_grid is not None:
                grid = self.cube_grid
            else:
                raise ValueError('generate_sampling_map needs res, or grid=')
        elif not isinstance(grid, CubeSphereGrid):
            raise TypeError('grid must be a DLWP.remap.CubeSphereGrid')
        if latlon is not None and not isinstance(latlon, LatLonGrid):
            raise TypeError('latlon must be a DLWP.remap.LatLonGrid')
        m = bilinear_map(grid, lat, lon, latlon=latlon, device=device)
        m.name = ('sample_CS%d_LL%dx%d' % (grid.N, latlon.n_lat, latlon.n_lon) if latlon is not None
                  else 'sample_CS%d_P%d' % (grid.N, m.n_b))
        if map_name is not None:
            write_offline_map(m, map_name)
        self.sampling_map = m
        return m

    def _sampling(self):
        if self.sampling_map is None:
            raise ValueError("No sampling map has been defined; use the 'generate_sampling_map' function first")
        return self.sampling_map

    def sample_array(self, x, axes=(-3, -2, -1), **missing):
        """
        Sample the cubed sphere with the sampling map: the (face, height, width) axes of x are replaced by (n,) for a point
        list or (lat, lon) for a lat-lon grid.  numpy input: host path, the input's float dtype.  HIP tensor (fp32 or bf16):
        fp32 device result, one launch.
        skipna, min_valid, renormalize, frac_out: NaN cells are missing values, left out of the sums (OfflineMap.apply).
        """
        return self._sampling().apply(x, axes, **_missing_kw(missing))

    def sample_forecast(self, forecast, **missing):
        """
        Sample a labelled cubed-sphere forecast (space dims as for inverse_remap_forecast).  A lat-lon sampling map gives what
        inverse_remap_forecast gives, smooth; a point list gives the dim 'point' with the coords 'lat' and 'lon' along it
        (`.lat` / `.lon` are Forecasts of dims ('point',)).  The values stay on the device when they came from there.
        skipna, min_valid, renormalize: NaN cells are missing values, left out of the sums (OfflineMap.apply).
        """
        missing = _missing_kw(missing, frac=False)
        m = self._sampling()
        dims = tuple(forecast.dims)
        a0 = _cube_axis(dims)
        vals = m.apply(forecast.values, (a0, a0 + 1, a0 + 2), **missing)
        grid = m.dst_kind == 'latlon'
        new_dims = dims[:a0] + (('lat', 'lon') if grid else ('point',)) + dims[a0 + 3:]
        coords = {d: c for d, c in forecast.coords.items() if d in new_dims}
        coords['lat'], coords['lon'] = (m.lat_b.copy(), m.lon_b.copy()) if grid else (m.yc_b.copy(), m.xc_b.copy())
        out = Forecast(vals, new_dims, coords, name=forecast.name)
        out.lat = Forecast(coords['lat'], ('lat',) if grid else ('point',), {'lat': coords['lat']}, name='lat')
        out.lon = Forecast(coords['lon'], ('lon',) if grid else ('point',), {'lon': coords['lon']}, name='lon')
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
