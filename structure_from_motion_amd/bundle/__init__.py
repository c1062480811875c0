"""Bundle adjustment: joint Levenberg-Marquardt refinement of camera poses and 3-D points (csrc/sfm_bundle.hip)."""
