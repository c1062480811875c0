"""Bundle adjustment of camera poses and 3-D points on the GPU (``sfm_bundle_adjust``).

Poses are ``R (9) | t (3)`` rows with ``x_cam = R X + t`` — the PnP model layout.  All cameras share one camera matrix
``K`` whose row 2 is (0, 0, 1); its focal length and principal point are refined on request (``refine_intrinsics``, the
dense solver only) and held otherwise.  The cost is the sum over the observations of rho(e), e the
squared reprojection error of the PnP scorer and rho the loss: ``"squared"`` (rho = e, the default), ``"huber"`` or
``"cauchy"`` with a scale in pixels.  Fixed cameras and points with fewer than two observations are held; with exactly
one fixed camera the scale is held by the distance from it to the lowest-index free camera.

Two linear solvers sit behind the same LM loop: ``"dense"`` factors the reduced camera system (at most 64 cameras,
DESIGN.md §6h) and ``"iterative"`` solves it by block-Jacobi preconditioned conjugate gradients without forming it (any
number of cameras, ``sfm_bundle_adjust_pcg``).
"""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np
import numpy.typing as npt

from .._native import BUNDLE_LOSSES as LOSSES
from .._native import bundle_refine_mask, loss_scale_ok
from ..pnp.pnp import check_camera_matrix

MAX_CAMERAS = 64   # of the dense solver
LINEAR_SOLVERS = ("dense", "iterative")
_INT32 = 2**31


def _array(value, name: str, shape: Tuple[int, ...]) -> npt.NDArray:
    a = np.asarray(value, dtype=np.float64)
    if a.ndim != len(shape) or any(want not in (-1, got) for want, got in zip(shape, a.shape)):
        raise ValueError(f"{name} must have shape {tuple('N' if s < 0 else s for s in shape)}, got {a.shape}")
    return a


def _indices(value, name: str, m: int) -> npt.NDArray:
    a = np.asarray(value)
    if a.shape != (m,):
        raise ValueError(f"{name} must have one entry per pixel ({m}), got shape {a.shape}")
    if m and not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{name} must be integers, got {a.dtype}")
    if m and (a.min() < -_INT32 or a.max() >= _INT32):
        raise ValueError(f"{name} must fit in 32 bits")
    return a.astype(np.int32)


def bundle_adjust(
    camera_matrix: npt.NDArray,
    poses: npt.NDArray,
    points_3d: npt.NDArray,
    camera_indices: Sequence[int],
    point_indices: Sequence[int],
    pixels: npt.NDArray,
    fixed_cameras: Sequence[int] = (0,),
    max_steps: int = 50,
    linear_solver: str = "dense",
    max_cg_iterations: int = 100,
    cg_tolerance: float = 0.1,
    loss: str = "squared",
    loss_scale: float = 1.0,
    refine_intrinsics: Sequence[str] = (),
):
    """Minimise the summed squared reprojection error over the free cameras' poses and the points.

    ``poses`` (C, 12), ``points_3d`` (P, 3); observation m is pixel ``pixels[m]`` of point ``point_indices[m]`` in camera
    ``camera_indices[m]``.  At most 64 cameras, at least one of them in ``fixed_cameras``; at most ``max_steps`` LM trial
    steps.  Returns ``(poses (C, 12), points (P, 3), info)`` with ``info`` a ``device.BundleInfo``.  An input whose cost
    is not finite (a point behind a camera), or an index out of range, comes back unchanged with ``info.status`` set
    (``device.BUNDLE_BAD_START`` / ``BUNDLE_BAD_INDEX``).  Every argument is checked before any device work.

    ``linear_solver="iterative"`` takes any number of cameras (at least 1) and solves each LM step's reduced camera
    system by preconditioned conjugate gradients: at most ``max_cg_iterations`` (>= 1) iterations, stopping once the
    residual is below ``cg_tolerance`` (in (0, 1)) times the right-hand side.  ``info`` is then a
    ``device.BundlePcgInfo`` (the ``BundleInfo`` fields plus ``cg_iterations`` and ``cg_max``).

    ``loss`` is one of ``LOSSES``.  With e an observation's squared reprojection error in px^2 and a = ``loss_scale`` in
    pixels (> 0 with a normal finite square, about 1.5e-154 to 1.3e154; no effect on ``"squared"``): ``"huber"`` is e up to a^2 and 2 a sqrt(e) - a^2 above, ``"cauchy"``
    is a^2 log1p(e / a^2).  ``info.initial_cost`` and ``info.final_cost`` are then the sums of rho(e), not of e, and the
    accept test and the stops use them.  Huber keeps a constant pull of 2 a per pixel on an outlier and suits moderate
    ones; Cauchy re-descends and suits gross ones.

    ``refine_intrinsics`` is a subset of ``("focal", "principal_point")``; empty (the default) holds ``camera_matrix`` and
    is the call described above.  ``"focal"`` frees f = K[0,0] (the 2 x 2 block of K is scaled as a whole, so the aspect
    ratio and the skew keep their proportions), ``"principal_point"`` frees K[0,2] and K[1,2] together; all cameras share
    them and ``camera_matrix`` is the start.  ``info`` is then a ``device.BundleCalibrationInfo``: the ``BundleInfo`` fields
    plus ``camera_matrix``, the refined K (the input K when ``info.status`` is not ``BUNDLE_OK``).  A scene must constrain
    what it frees: cameras that converge on the points do, nearly parallel ones leave the focal length loose (DESIGN.md
    §6ab).  Only the dense solver refines intrinsics: with ``linear_solver="iterative"`` a non-empty value is a ValueError."""
    K = check_camera_matrix(camera_matrix)
    poses = _array(poses, "poses", (-1, 12))
    points = _array(points_3d, "points_3d", (-1, 3))
    pixels = _array(pixels, "pixels", (-1, 2))
    m = pixels.shape[0]
    cams = _indices(camera_indices, "camera_indices", m)
    pts = _indices(point_indices, "point_indices", m)
    n_cams = poses.shape[0]
    if linear_solver not in LINEAR_SOLVERS:
        raise ValueError(f"linear_solver must be one of {LINEAR_SOLVERS}, got {linear_solver!r}")
    iterative = linear_solver == "iterative"
    if iterative:
        if n_cams < 1 or n_cams >= _INT32:
            raise ValueError(f"the iterative solver needs between 1 and 2^31 - 1 cameras, got {n_cams}")
        if (isinstance(max_cg_iterations, bool) or not isinstance(max_cg_iterations, (int, np.integer))
                or not 1 <= max_cg_iterations < _INT32):
            raise ValueError(f"max_cg_iterations must be a positive integer, got {max_cg_iterations!r}")
        if (isinstance(cg_tolerance, bool) or not isinstance(cg_tolerance, (int, float, np.floating))
                or not 0.0 < float(cg_tolerance) < 1.0):
            raise ValueError(f"cg_tolerance must be a number in (0, 1), got {cg_tolerance!r}")
    elif not 1 <= n_cams <= MAX_CAMERAS:
        raise ValueError(f"between 1 and {MAX_CAMERAS} cameras are supported, got {n_cams}")
    if points.shape[0] >= _INT32 or m >= _INT32:
        raise ValueError("points and observations must number fewer than 2^31")
    fixed = [int(c) for c in fixed_cameras]
    if not fixed:
        raise ValueError("at least one camera must be fixed")
    if any(not 0 <= c < n_cams for c in fixed) or len(set(fixed)) != len(fixed):
        raise ValueError(f"fixed_cameras must be distinct camera indices in [0, {n_cams}), got {fixed}")
    if isinstance(max_steps, bool) or not isinstance(max_steps, (int, np.integer)) or max_steps < 0:
        raise ValueError(f"max_steps must be a non-negative integer, got {max_steps!r}")
    if not isinstance(loss, str) or loss not in LOSSES:
        raise ValueError(f"loss must be one of {LOSSES}, got {loss!r}")
    if (isinstance(loss_scale, bool) or not isinstance(loss_scale, (int, float, np.integer, np.floating))
            or not loss_scale_ok(float(loss_scale))):
        raise ValueError(f"loss_scale must be a number > 0 with a normal finite square, got {loss_scale!r}")
    refine = bundle_refine_mask(refine_intrinsics)
    if refine and iterative:
        raise ValueError("refine_intrinsics needs linear_solver=\"dense\": the iterative solver holds the camera matrix")
    if refine & 1 and K[0, 0] == 0.0:
        raise ValueError("camera_matrix[0, 0] is zero: the focal length cannot be refined")
    import torch

    from .. import device

    device.require_gpu()
    if refine:
        poses_d, points_d, info, K_d = device.bundle_adjust_calibrated(
            device.to_device(poses), device.to_device(points), device.to_device(cams, dtype=torch.int32),
            device.to_device(pts, dtype=torch.int32), device.to_device(pixels), K, fixed, int(max_steps),
            refine=list(refine_intrinsics), loss=loss, loss_scale=float(loss_scale))
        return poses_d.cpu().numpy(), points_d.cpu().numpy(), device.read_bundle_calibration_info(info, K_d)
    robust = {} if loss == "squared" else dict(loss=loss, loss_scale=float(loss_scale))   # squared: today's call
    if iterative:
        poses_d, points_d, info = device.bundle_adjust_pcg(
            device.to_device(poses), device.to_device(points), device.to_device(cams, dtype=torch.int32),
            device.to_device(pts, dtype=torch.int32), device.to_device(pixels), K, fixed, int(max_steps),
            int(max_cg_iterations), float(cg_tolerance), **robust)
        return poses_d.cpu().numpy(), points_d.cpu().numpy(), device.read_bundle_pcg_info(info)
    poses_d, points_d, info = device.bundle_adjust(
        device.to_device(poses), device.to_device(points), device.to_device(cams, dtype=torch.int32),
        device.to_device(pts, dtype=torch.int32), device.to_device(pixels), K, fixed, int(max_steps), **robust)
    return poses_d.cpu().numpy(), points_d.cpu().numpy(), device.read_bundle_info(info)
