"""``lib.multiview.track_refinement`` — sub-pixel refinement of track observations, re-exported from ``structure_from_motion_amd.multiview.track_refinement``."""
from structure_from_motion_amd.multiview.track_refinement import (TrackRefinement, bin_rotation, level_pixels,  # noqa: F401
                                                                  refine_observations, refine_track_observations,
                                                                  track_references)
