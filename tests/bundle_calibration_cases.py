"""Scenes and the stream case of the calibrating bundle adjuster (sfm_bundle_adjust_calibrated).

``ring_problem`` is the scene on which shared intrinsics are observable: ``synthetic.bundle_problem``'s nearly parallel
cameras leave the focal length loose (it trades against depth), cameras that converge on the points do not.

Importing this module registers the stream case of the new entry point in ``stream_cases.CASES``; the two test files of
the feature import it at their top and sort before test_gpu_streams.py and test_stream_cases_host.py, so both of those see
the complete table in a run of the whole suite."""
import ctypes as C
import functools

import numpy as np

import stream_cases

RING_K = np.array([[800.0, 0.0, 320.0], [0.0, 810.0, 240.0], [0.0, 0.0, 1.0]])


def look_at_origin(centre):
    """R (3, 3), t (3,) of a camera at ``centre`` whose optical axis passes through the origin (y roughly up)."""
    z = -centre / np.linalg.norm(centre)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    return R, -R @ centre


def ring_problem(cameras, points, per_point=4, seed=0, noise_px=0.5, K=RING_K, rotation_noise=0.003,
                 translation_noise=0.01, point_noise=0.01):
    """A converging ring: camera centres at radius 5, spread over +-50 degrees about y, heights alternating +-0.8, every
    camera looking at the origin; points uniform in [-1, 1]^3, each seen by min(per_point, cameras) cameras with Gaussian
    pixel noise.  The start perturbs every camera but camera 0 and every point, as ``synthetic.bundle_problem`` does.
    Returns its dict; ``K`` is the true camera matrix."""
    from structure_from_motion_amd import synthetic

    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 1.0, (points, 3))
    poses = np.zeros((cameras, 12))
    for c in range(cameras):
        a = np.radians(-50.0 + 100.0 * c / max(cameras - 1, 1))
        R, t = look_at_origin(np.array([5.0 * np.sin(a), 0.8 if c % 2 == 0 else -0.8, -5.0 * np.cos(a)]))
        poses[c] = np.concatenate([R.reshape(9), t])
    k = min(per_point, cameras)
    cam = np.argsort(rng.random((points, cameras)), axis=1)[:, :k].reshape(-1)
    pt = np.repeat(np.arange(points), k)
    order = rng.permutation(len(cam))
    cam, pt = cam[order], pt[order]
    xc = np.einsum("mij,mj->mi", poses[cam, :9].reshape(-1, 3, 3), X[pt]) + poses[cam, 9:]
    uvw = xc @ K.T
    pixels = uvw[:, :2] / uvw[:, 2:3] + rng.normal(0.0, noise_px, (len(cam), 2))
    start = poses.copy()
    for c in range(1, cameras):
        start[c, :9] = (synthetic._small_rotation(rng, rotation_noise) @ poses[c, :9].reshape(3, 3)).reshape(9)
        start[c, 9:] += rng.normal(0.0, translation_noise, 3)
    return dict(K=K.copy(), poses=start, points=X + rng.normal(0.0, point_noise, X.shape), camera_indices=cam.astype(np.int32),
                point_indices=pt.astype(np.int32), pixels=pixels, poses_true=poses, points_true=X)


def wrong_camera(K, focal_error=0.05, centre_shift=(0.0, 0.0)):
    """K with its 2 x 2 block scaled by 1 + focal_error and its principal point moved by centre_shift pixels."""
    K = np.array(K, dtype=np.float64)
    K[:2, :2] *= 1.0 + focal_error
    K[0, 2] += centre_shift[0]
    K[1, 2] += centre_shift[1]
    return K


SKEW_K = np.array([[800.0, 2.0, 320.0], [1.5, 810.0, 240.0], [0.0, 0.0, 1.0]])
# LM steps of the device-against-oracle cases.  A parity case needs every accept test decided well above rounding, or the
# device and the oracle may rightly part there: the oracle's trial cost differs from the current cost by at least
# MIN_MARGIN of it at every step (test_bundle_calibration_host.py checks it), and every case still accepts three steps.  At
# five steps three of the cases below test a decrease of 1e-13 or less of the cost.
PARITY_STEPS = 4
MIN_MARGIN = 1e-10


def _case(pr, fixed=(0,), refine=("focal", "principal_point"), **loss):
    """A parity case: the problem, started from a camera matrix 5 % and (10, -6) px off."""
    return dict(pr=pr, K=wrong_camera(pr["K"], 0.05, (10.0, -6.0)), fixed=fixed, refine=refine, loss=loss)


def _with_single_observation_points(pr, count):
    """``pr`` where points 0 .. count - 1 keep only their first observation: they are held."""
    pt = pr["point_indices"]
    first = np.zeros(len(pt), dtype=bool)
    first[np.unique(pt, return_index=True)[1]] = True
    keep = (pt >= count) | first
    return dict(pr, camera_indices=pr["camera_indices"][keep], point_indices=pt[keep], pixels=pr["pixels"][keep])


@functools.lru_cache(maxsize=None)
def parity_cases():
    """name -> dict(pr, K, fixed, refine, loss): the smallest shapes that reach every branch of the calibrating kernels.
    Each refine mask; two fixed cameras (observations in fixed cameras, no gauge rescale); 31 free cameras (the reduced
    system in global memory); held points; both robust losses; a camera matrix with skew."""
    return {
        "3x24_focal": _case(ring_problem(3, 24, seed=11), refine=("focal",)),
        "3x24_principal_point": _case(ring_problem(3, 24, seed=11), refine=("principal_point",)),
        "3x24_all": _case(ring_problem(3, 24, seed=11)),
        "4x40_two_fixed": _case(ring_problem(4, 40, seed=12), fixed=(0, 2)),
        "32x200_global_solve": _case(ring_problem(32, 200, seed=13)),
        "5x60_held_points": _case(_with_single_observation_points(ring_problem(5, 60, seed=25), 9)),
        "5x60_huber": _case(ring_problem(5, 60, seed=15), loss="huber", loss_scale=0.7),
        "5x60_cauchy": _case(ring_problem(5, 60, seed=16), loss="cauchy", loss_scale=1.0),
        "5x60_skew": _case(ring_problem(5, 60, seed=17, K=SKEW_K)),
    }


# The largest difference between the oracle's Schur and dense solvers over the parity cases after PARITY_STEPS steps,
# measured on the CPU (test_bundle_calibration_host.py re-measures it; profiles/bundle_calibration/README.md): the absolute
# difference of poses, points and K, the relative one of the final cost.  The device is allowed ten times as much.
# Measured: poses 3.47e-12, points 1.33e-11, K 1.75e-9, cost 3.58e-12 (all four on 5x60_cauchy); rounded up.
SPREAD = dict(poses=3.5e-12, points=1.4e-11, K=1.8e-9, cost=3.6e-12)
DEVICE_TOLERANCE = {k: 10.0 * v for k, v in SPREAD.items()}
# The relative focal error the oracle itself ends with on the noise-free ring (6 x 96, 5 % off, the focal length free):
# 7.15e-13, 6.43e-13 and 8.74e-13 on seeds 0, 1 and 2; rounded up.
EXACT_FOCAL = 8.8e-13


@stream_cases.case(["sfm_bundle_adjust_calibrated"], ["bundle_adjust_calibrated_"])
def bundle_adjust_calibrated(dev):
    """6 cameras x 96 points of the ring from a camera matrix 5 % and (10, -6) px off, three steps: the C entry point with
    all three intrinsics free on the test's workspace, and the in-place op with the focal length free under Huber."""
    import torch

    from structure_from_motion_amd import _native, device

    cameras, points, max_steps = 6, 96, 3
    i = stream_cases.Inst(dev)
    a, b = ring_problem(cameras, points, seed=0), ring_problem(cameras, points, seed=1)
    M = len(a["pixels"])
    assert M == len(b["pixels"])
    keys = ("poses", "points", "camera_indices", "point_indices", "pixels")
    poses, pts, cam, pt, pix = (i.inp(a[k], b[k]) for k in keys)
    K = wrong_camera(RING_K, 0.05, (10.0, -6.0))

    def outputs(tag):
        return [i.out("poses" + tag, (cameras, 12), torch.float64), i.out("points" + tag, (points, 3), torch.float64),
                i.out("info" + tag, (4,), torch.int64), i.out("K_out" + tag, (3, 3), torch.float64)]
    plain, op = outputs(""), outputs("_op")
    lib = stream_cases._lib()
    ws = i.work(lib.sfm_bundle_calibrated_workspace_bytes(cameras, points, M))
    options = _native.BundleCalibrationOptions(_native.BundleOptions(0, 0, 1.0), 3, 0)
    Kc = (C.c_double * 9)(*[float(v) for v in K.reshape(9)])
    fixed = (C.c_uint8 * cameras)(1, *([0] * (cameras - 1)))
    i.keep = (Kc, fixed, options)

    def call():
        stream_cases._check(lib.sfm_bundle_adjust_calibrated(
            C.cast(Kc, C.c_void_p), cameras, points, M, C.cast(fixed, C.c_void_p), poses.data_ptr(), pts.data_ptr(),
            cam.data_ptr(), pt.data_ptr(), pix.data_ptr(), max_steps, plain[0].data_ptr(), plain[1].data_ptr(),
            plain[2].data_ptr(), plain[3].data_ptr(), ws.data_ptr(), ws.numel(), stream_cases._st(), C.byref(options)),
            "sfm_bundle_adjust_calibrated")
        op[0].copy_(poses), op[1].copy_(pts)
        device.bundle_adjust_calibrated(op[0], op[1], cam, pt, pix, K, (0,), max_steps, out=tuple(op), refine=("focal",),
                                        loss="huber", loss_scale=2.0)
    i.call = call
    return i
