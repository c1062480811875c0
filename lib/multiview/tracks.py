"""``lib.multiview.tracks`` — triangulation of multi-view tracks and tracks from pairwise matches, re-exported from ``structure_from_motion_amd.multiview.tracks``."""
from structure_from_motion_amd.multiview.tracks import (TrackBuildResult, TracksResult, build_tracks,  # noqa: F401
                                                        triangulate_tracks)
