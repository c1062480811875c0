"""``lib.multiview.tracks`` — triangulation of multi-view tracks, re-exported from ``structure_from_motion_amd.multiview.tracks``."""
from structure_from_motion_amd.multiview.tracks import TracksResult, triangulate_tracks  # noqa: F401
