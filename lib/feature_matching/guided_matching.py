"""``lib.feature_matching.guided_matching``: descriptor matching guided by the verified two-view models of a view graph (no
counterpart in the reference)."""
from structure_from_motion_amd.feature_matching.guided_matching import (  # noqa: F401
    guided_match_models,
    guided_match_pairs,
)
