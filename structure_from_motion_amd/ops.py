"""``torch.ops.sfm_hip.*`` — the hot-path kernels as PyTorch-ROCm custom ops (csrc/sfm_torch_ops.cpp, a
``TORCH_LIBRARY`` above the C ABI of include/sfm_hip.h).

The ``TORCH_LIBRARY(sfm_hip, m)`` block of that file is the list of ops and their schemas.  A functional op allocates its
outputs and has a Meta form (fake tensors, ``torch.compile``, ``torch.library.opcheck``); an in-place ``*_`` op writes the
buffers the pre-allocating engine hands it.  ``device.py`` dispatches through them; ``load()`` must have run before
``torch.ops.sfm_hip`` is touched.
"""
from __future__ import annotations

import os

import torch

from . import _native

HERE = os.path.dirname(os.path.abspath(__file__))
OPS_LIB_PATH = os.path.join(HERE, "csrc", "libsfm_torch_ops.so")

_loaded = False


def load():
    """Load libsfm_hip.so and register the ``sfm_hip`` op library with torch (idempotent).  Raises if either
    library is missing: there is no Python or CPU fallback for these ops."""
    global _loaded
    if not _loaded:
        _native.load()
        if not os.path.exists(OPS_LIB_PATH):
            raise _native.NativeLibraryError(
                f"{OPS_LIB_PATH} is missing: build it with `python -m structure_from_motion_amd.build`")
        import ctypes

        ops_abi = ctypes.CDLL(OPS_LIB_PATH).sfm_torch_ops_abi_version()   # the C-ABI version it was compiled against
        if ops_abi != _native.ABI_VERSION:
            raise _native.NativeLibraryError(
                f"libsfm_torch_ops.so was built against C-ABI {ops_abi}, libsfm_hip.so is {_native.ABI_VERSION}; "
                f"rebuild both with `python -m structure_from_motion_amd.build --force`")
        torch.ops.load_library(OPS_LIB_PATH)
        _loaded = True
    return torch.ops.sfm_hip


FUNCTIONAL_OPS = ("normalize_coords", "sample_philox", "fit_eight_point", "score_sed", "select_best", "inlier_mask",
                  "cheirality", "triangulate", "five_point_fit", "homography_fit", "homography_score", "homography_inlier_mask", "pair_poses", "pnp_fit", "p3p_fit", "pnp_score", "pnp_refine", "bundle_adjust", "bundle_adjust_pcg",
                  "triangulate_tracks", "build_tracks", "bundle_adjust_robust", "bundle_adjust_pcg_robust", "average_rotations",
                  "average_translations", "bundle_adjust_calibrated")
INPLACE_OPS = ("normalize_coords_", "fit_eight_point_", "sample_fit_philox_", "score_sed_", "select_best_",
               "inlier_mask_", "ransac_pass_small_", "five_point_fit_", "five_point_ransac_pass_", "homography_ransac_pass_", "verify_pairs_", "pnp_fit_", "p3p_fit_", "pnp_score_", "pnp_ransac_pass_", "p3p_ransac_pass_", "pnp_refine_", "bundle_adjust_", "bundle_adjust_pcg_",
               "triangulate_tracks_", "build_tracks_", "bundle_adjust_robust_", "bundle_adjust_pcg_robust_",
               "bundle_adjust_calibrated_")
# The two tuples above are the op set whose schemas tests/golden/op_schemas_before_calibration.json pins (plus the calibrating
# adjuster, which that guard names): an op added since is listed here, so that the guard keeps comparing what it was written for.
LATER_FUNCTIONAL_OPS = ("refine_pair_poses",)
# the ragged absolute-pose call, functional and in place: listed beside the pinned tuples like the one above
REGISTER_VIEWS_OPS = ("register_views", "register_views_")
# the similarity alignment of two reconstructions, each functional and in place: listed beside them too
SIMILARITY_OPS = ("similarity_ransac_pass", "similarity_ransac_pass_", "similarity_fit", "similarity_fit_", "similarity_refine",
                  "similarity_refine_")
# the ragged alignment of every pair of sub-models, functional and in place: listed beside them as well
ALIGN_MODELS_OPS = ("align_models", "align_models_")
# plane-sweep depth maps and their consistency filter, functional and in place: listed beside them as well
DEPTH_MAP_OPS = ("plane_sweep", "plane_sweep_", "filter_depth_maps", "filter_depth_maps_")
# fusion of depth maps into a TSDF volume and its mesh, functional and in place: listed beside them as well
FUSION_OPS = ("tsdf_integrate", "tsdf_integrate_", "tsdf_extract_mesh", "tsdf_extract_mesh_")
# semi-global smoothing of the plane-sweep cost volume, functional and in place: listed beside them as well
SGM_OPS = ("sgm_aggregate", "sgm_aggregate_")
