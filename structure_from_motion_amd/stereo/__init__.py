"""Dense stereo: plane-sweep depth maps from posed images and their consistency filter (csrc/sfm_plane_sweep.hip), and their
fusion into a TSDF volume and a triangle mesh (csrc/sfm_tsdf.hip)."""
