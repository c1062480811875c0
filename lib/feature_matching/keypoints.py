"""``lib.feature_matching.keypoints``: multi-scale FAST keypoints with BRIEF per pyramid level for a whole collection (no
counterpart in the reference)."""
from structure_from_motion_amd.feature_matching.keypoints import (  # noqa: F401
    ImageKeypoints,
    detect_and_describe,
)
