"""``lib.multiview.tracks`` — triangulation of multi-view tracks (plain and outlier-robust) and tracks from pairwise matches, re-exported from ``structure_from_motion_amd.multiview.tracks``."""
from structure_from_motion_amd.multiview.tracks import (RobustTracksResult, TrackBuildResult, TracksResult,  # noqa: F401
                                                        build_tracks, triangulate_tracks, triangulate_tracks_robust)
