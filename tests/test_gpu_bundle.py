"""Bundle adjustment on the MI355X (csrc/sfm_bundle.hip): parity with the NumPy oracle of tests/bundle_oracle.py from
3 x 200 to 16 x 20 000 (both homes of the reduced camera system: LDS and global memory), determinism, the gauge and edge
cases, the op layer, and the three-view app."""
import numpy as np
import pytest
import torch

import bundle_oracle as bo
from structure_from_motion_amd import synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(native_lib):
    from structure_from_motion_amd import device

    return device.require_gpu()


def _problem(C, P, seed, per_point=4):
    return synthetic.bundle_problem(C, P, per_point=per_point, seed=seed)


def _device_call(pr, fixed=(0,), max_steps=50, poses=None, points=None, cam=None, pt=None):
    from structure_from_motion_amd import device

    out = device.bundle_adjust(device.to_device(pr["poses"] if poses is None else poses),
                               device.to_device(pr["points"] if points is None else points),
                               device.to_device(pr["camera_indices"] if cam is None else cam, dtype=torch.int32),
                               device.to_device(pr["point_indices"] if pt is None else pt, dtype=torch.int32),
                               device.to_device(pr["pixels"]), pr["K"], fixed, max_steps)
    return out[0].cpu().numpy(), out[1].cpu().numpy(), device.read_bundle_info(out[2])


def _oracle(pr, fixed=(0,), max_steps=50):
    return bo.adjust(pr["K"], pr["poses"], pr["points"], pr["camera_indices"], pr["point_indices"], pr["pixels"],
                     fixed=fixed, max_steps=max_steps)


# The device and the oracle take the same LM path (the same accepted steps) and differ in the summation order only.  Over
# these sizes the final estimates agree to 3e-15 (poses) and 6e-14 (points, 4-6 units from the cameras); the estimate
# itself moves by 2e-2 .. 7e-2.  1e-10 leaves three orders of margin for other seeds and still catches any difference in
# the algorithm (a different step, damping or gauge rule moves the result by far more).
POSE_TOL = 1e-10
POINT_TOL = 1e-10


@pytest.mark.parametrize("C,P,seed", [(3, 200, 11), (8, 2000, 12), (16, 20000, 13), (40, 3000, 14), (64, 2000, 15)])
def test_parity_with_oracle(dev, C, P, seed):
    """(40, 3000) and (64, 2000) have more free cameras than the LDS holds: S lives in global memory there."""
    pr = _problem(C, P, seed)
    poses, points, info = _device_call(pr)
    ref = _oracle(pr)
    assert info.status == ref["status"] == 0
    assert info.accepted == ref["accepted"] and info.accepted >= 3, (info, ref["accepted"], ref["steps"])
    assert abs(info.initial_cost - ref["initial_cost"]) <= 1e-12 * ref["initial_cost"]
    assert abs(info.final_cost - ref["final_cost"]) <= 1e-9 * ref["final_cost"], (info.final_cost, ref["final_cost"])
    assert info.final_cost < 0.01 * info.initial_cost
    assert np.max(np.abs(poses - ref["poses"])) <= POSE_TOL, np.max(np.abs(poses - ref["poses"]))
    assert np.max(np.abs(points - ref["points"])) <= POINT_TOL, np.max(np.abs(points - ref["points"]))


def test_bit_identical_across_calls(dev):
    pr = _problem(16, 20000, 21)
    a = _device_call(pr)
    b = _device_call(pr)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[2] == b[2]


def test_gauge_fixed_camera_and_anchor_distance(dev):
    pr = _problem(6, 1000, 22)
    poses, points, info = _device_call(pr, fixed=(2,))
    assert info.accepted >= 1
    assert np.array_equal(poses[2], pr["poses"][2])
    c0 = bo.centre(pr["poses"][2])
    before = np.linalg.norm(bo.centre(pr["poses"][0]) - c0)
    after = np.linalg.norm(bo.centre(poses[0]) - c0)
    assert abs(after - before) <= 1e-12 * before


def test_max_steps_zero_returns_input(dev):
    pr = _problem(5, 500, 23)
    poses, points, info = _device_call(pr, max_steps=0)
    assert np.array_equal(poses, pr["poses"]) and np.array_equal(points, pr["points"])
    assert info.steps == 0 and info.accepted == 0 and info.status == 0
    assert info.initial_cost == info.final_cost > 0.0


def test_all_but_one_fixed_moves_only_points_and_free_camera(dev):
    pr = _problem(5, 800, 24)
    fixed = (0, 1, 3, 4)
    poses, points, info = _device_call(pr, fixed=fixed)
    ref = _oracle(pr, fixed=fixed)
    assert info.accepted == ref["accepted"] >= 1
    for c in fixed:
        assert np.array_equal(poses[c], pr["poses"][c])
    assert not np.array_equal(poses[2], pr["poses"][2])
    assert np.max(np.abs(poses - ref["poses"])) <= POSE_TOL
    assert np.max(np.abs(points - ref["points"])) <= POINT_TOL


def test_single_observation_point_is_held(dev):
    pr = _problem(4, 300, 25)
    keep = pr["point_indices"] != 7
    first = np.nonzero(~keep)[0][0]
    keep[first] = True   # point 7 keeps one observation
    cam, pt, pix = pr["camera_indices"][keep], pr["point_indices"][keep], pr["pixels"][keep]
    sub = dict(pr, camera_indices=cam, point_indices=pt, pixels=pix)
    # two fixed cameras: no gauge rescale, so a held point is bit-unchanged
    poses, points, info = _device_call(sub, fixed=(0, 1))
    assert info.accepted >= 1
    assert np.array_equal(points[7], pr["points"][7])
    # one fixed camera: the gauge rescale about camera 0's centre (the origin) moves it along its ray, as in the oracle
    poses, points, info = _device_call(sub)
    ref = _oracle(sub)
    assert info.accepted == ref["accepted"] >= 1
    assert np.max(np.abs(points - ref["points"])) <= POINT_TOL
    assert np.linalg.norm(np.cross(points[7], pr["points"][7])) <= 1e-12 * np.linalg.norm(pr["points"][7]) ** 2


def test_non_finite_start_and_bad_index_leave_input(dev):
    from structure_from_motion_amd import device

    pr = _problem(4, 300, 26)
    behind = pr["points"].copy()
    behind[5, 2] = -3.0   # behind every camera
    poses, points, info = _device_call(pr, points=behind)
    assert info.status == device.BUNDLE_BAD_START and info.steps == 0
    assert np.isinf(info.initial_cost)
    assert np.array_equal(poses, pr["poses"]) and np.array_equal(points, behind)
    for cam, pt in ((None, pr["point_indices"].copy()), (pr["camera_indices"].copy(), None)):
        bad_cam = pr["camera_indices"] if cam is None else cam
        bad_pt = pr["point_indices"] if pt is None else pt
        if cam is None:
            bad_pt[17] = 300
        else:
            bad_cam[17] = -1
        poses, points, info = _device_call(pr, cam=bad_cam, pt=bad_pt)
        assert info.status == device.BUNDLE_BAD_INDEX and info.steps == 0
        assert np.array_equal(poses, pr["poses"]) and np.array_equal(points, pr["points"])


def test_inplace_op_matches_functional(dev):
    from structure_from_motion_amd import device, ops

    pr = _problem(5, 1000, 27)
    poses, points, info = _device_call(pr)
    P = device.to_device(pr["poses"])
    X = device.to_device(pr["points"])
    rec = torch.empty(4, dtype=torch.int64, device=dev)
    ops.load()
    device.bundle_adjust(None, None, device.to_device(pr["camera_indices"], dtype=torch.int32),
                         device.to_device(pr["point_indices"], dtype=torch.int32), device.to_device(pr["pixels"]), pr["K"],
                         out=(P, X, rec))
    assert np.array_equal(P.cpu().numpy(), poses) and np.array_equal(X.cpu().numpy(), points)
    assert device.read_bundle_info(rec) == info


def test_public_api_matches_device(dev):
    from lib.bundle.bundle import bundle_adjust

    pr = _problem(4, 400, 28)
    poses, points, info = bundle_adjust(pr["K"], pr["poses"], pr["points"], pr["camera_indices"].astype(np.int64),
                                        pr["point_indices"], pr["pixels"], fixed_cameras=(0,), max_steps=30)
    ref = _device_call(pr, max_steps=30)
    assert np.array_equal(poses, ref[0]) and np.array_equal(points, ref[1]) and info == ref[2]


def test_three_view_app_bundle_adjust_lowers_r2_error(dev):
    """The feature: on the noisy three-view scene, adjusting all three views and the points lowers view 2's rotation error
    below what the two-view reconstruction alone gives, and does not raise the cost."""
    from apps import sfm_three_view

    kw = dict(n=400, seed=11, noise_px=0.5, sed_threshold=6e-6, reprojection_threshold=4.0)
    plain = sfm_three_view.run(**kw)
    adjusted = sfm_three_view.run(**kw, bundle_adjust=30)
    assert adjusted["R2_error_rad_before_ba"] == plain["R2_error_rad"]
    assert adjusted["R2_error_rad"] < plain["R2_error_rad"]
    assert adjusted["R3_error_rad"] < plain["R3_error_rad"]
    assert adjusted["rms_px"] <= adjusted["rms_px_before_ba"]
    assert adjusted["ba_status"] == 0 and adjusted["ba_accepted"] >= 1
