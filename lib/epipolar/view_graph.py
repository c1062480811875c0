"""``lib.epipolar.view_graph``: two-view verification of every pair of a match graph in one device call and the choice of the seed pair (structure_from_motion_amd/epipolar/view_graph.py)."""
from structure_from_motion_amd.epipolar.view_graph import (  # noqa: F401
    PairPoses,
    PairRefinement,
    ViewGraph,
    choose_seed_pair,
    chunk_bounds,
    pair_min_extra,
    refine_relative_poses,
    verify_pairs,
)
