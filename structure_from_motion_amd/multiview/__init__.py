"""Multi-view structure: points triangulated from tracks of two or more views (csrc/sfm_tracks.hip)."""
