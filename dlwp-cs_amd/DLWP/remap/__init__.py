"""
Remapping between the cubed sphere and lat-lon grids with offline maps (reference DLWP/remap).  Maps are read from netCDF
classic / 64-bit-offset files (read_offline_map), built from arrays (OfflineMap) or generated in closed form from the two grids
(CubeSphereRemap.generate_maps, conservative_maps) and applied to arrays: device tensors by the dlwpcs_sparse_map_apply
kernel, numpy arrays on the host.  Bilinear sampling maps from the cube to arbitrary points or a fine lat-lon grid (bilinear_map,
point_weights, CubeSphereRemap.generate_sampling_map) are OfflineMaps as well and are applied by the same kernel.
"""
from .cubesphere import CubeSphereRemap
from .grid import CubeSphereGrid, LatLonGrid
from .offline_map import OfflineMap, read_offline_map, write_offline_map
from .overlap import conservative_maps, overlap_areas
from .bilinear import bilinear_map, dual_faces, point_weights

__all__ = ['CubeSphereRemap', 'CubeSphereGrid', 'LatLonGrid', 'OfflineMap', 'read_offline_map', 'write_offline_map',
           'conservative_maps', 'overlap_areas', 'bilinear_map', 'dual_faces', 'point_weights']
