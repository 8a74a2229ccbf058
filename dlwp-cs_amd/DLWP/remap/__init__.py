"""
Remapping between the cubed sphere and lat-lon grids with offline maps (reference DLWP/remap).  Maps are read from netCDF
classic / 64-bit-offset files (read_offline_map) or built from arrays (OfflineMap) and applied to arrays: device tensors by the
dlwpcs_sparse_map_apply kernel, numpy arrays on the host.
"""
from .cubesphere import CubeSphereRemap
from .offline_map import OfflineMap, read_offline_map

__all__ = ['CubeSphereRemap', 'OfflineMap', 'read_offline_map']
