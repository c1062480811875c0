"""``lib.stereo.fusion`` — depth maps fused into a TSDF volume and its triangle mesh, re-exported from ``structure_from_motion_amd.stereo.fusion``."""
from structure_from_motion_amd.stereo.fusion import (Mesh, TsdfVolume, fuse_depth_maps, save_ply, suggest_voxel_size,  # noqa: F401
                                                     volume_bounds)
