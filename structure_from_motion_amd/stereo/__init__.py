"""Dense stereo: plane-sweep depth maps from posed images and their consistency filter (csrc/sfm_plane_sweep.hip)."""
