"""``lib.multiview.alignment`` — similarity alignment of reconstructions, re-exported from ``structure_from_motion_amd.multiview.alignment``."""
from structure_from_motion_amd.multiview.alignment import (ModelAlignments, ModelFrames, SimilarityCalculationError,  # noqa: F401
                                                           SimilarityEstimate, align_models, apply_similarity, compose,
                                                           estimate_similarity_with_ransac, fit_similarity,
                                                           inconsistent_alignments, invert, merge_frames, transform_poses)
