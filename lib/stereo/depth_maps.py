"""``lib.stereo.depth_maps`` — plane-sweep depth maps, their semi-global smoothing and their consistency filter, re-exported from ``structure_from_motion_amd.stereo.depth_maps``."""
from structure_from_motion_amd.stereo.depth_maps import (DepthMaps, FilteredDepthMaps, compute_depth_maps, depth_hypotheses,  # noqa: F401
                                                         depth_ranges, filter_depth_maps, point_cloud, regularize_depth_maps,
                                                         select_source_views)
