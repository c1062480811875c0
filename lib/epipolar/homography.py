"""``lib.epipolar.homography``: RANSAC homography and the two-view model choice (structure_from_motion_amd/epipolar/homography.py)."""
from structure_from_motion_amd.epipolar.homography import (  # noqa: F401
    FeaturePair,
    HomographyCalculationError,
    TwoViewModel,
    calculate_transfer_error_score,
    estimate_homography_with_ransac,
    homography_model_fitter,
    select_two_view_model,
)
