"""``lib.pnp.pnp``: RANSAC absolute pose (structure_from_motion_amd/pnp/pnp.py)."""
from structure_from_motion_amd.pnp.pnp import (  # noqa: F401
    PnPCalculationError,
    calculate_reprojection_score,
    estimate_pose_pnp_with_ransac,
    p3p_model_fitter,
    pnp_model_fitter,
    refine_pose_pnp,
)
