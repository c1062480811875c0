"""``lib.feature_matching.graph_matching``: descriptor matching of every image pair of a collection (no counterpart in the
reference)."""
from structure_from_motion_amd.feature_matching.graph_matching import (  # noqa: F401
    PairMatches,
    all_pairs,
    match_image_pairs,
)
