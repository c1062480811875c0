"""``lib.feature_matching.brief``: oriented BRIEF descriptors and their Hamming score (no counterpart in the reference)."""
from structure_from_motion_amd.feature_matching.brief import (  # noqa: F401
    BriefDescriptors,
    BriefScore,
    compute_brief,
    load_pattern,
)
