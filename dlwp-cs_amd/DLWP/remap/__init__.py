"""
Remapping between the cubed sphere and lat-lon grids with offline maps (reference DLWP/remap).  Maps are read from netCDF
classic / 64-bit-offset files (read_offline_map), built from arrays (OfflineMap) or generated in closed form from the two grids
(CubeSphereRemap.generate_maps, conservative_maps) and applied to arrays: device tensors by the dlwpcs_sparse_map_apply
kernel, numpy arrays on the host.
"""
from .cubesphere import CubeSphereRemap
from .grid import CubeSphereGrid, LatLonGrid
from .offline_map import OfflineMap, read_offline_map, write_offline_map
from .overlap import conservative_maps, overlap_areas

__all__ = ['CubeSphereRemap', 'CubeSphereGrid', 'LatLonGrid', 'OfflineMap', 'read_offline_map', 'write_offline_map',
           'conservative_maps', 'overlap_areas']
