"""``lib.multiview.alignment`` — similarity alignment of two reconstructions, re-exported from ``structure_from_motion_amd.multiview.alignment``."""
from structure_from_motion_amd.multiview.alignment import (SimilarityCalculationError, SimilarityEstimate,  # noqa: F401
                                                           apply_similarity, compose, estimate_similarity_with_ransac,
                                                           fit_similarity, invert, transform_poses)
