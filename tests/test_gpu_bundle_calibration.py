"""The calibrating bundle adjuster on the MI355X (sfm_bundle_adjust_calibrated): parity with the NumPy
oracle of tests/bundle_calibration_oracle.py on the smallest shapes that reach every branch, the statuses, bit
reproducibility, the empty ``refine_intrinsics`` against the call without it, and the recovery of a wrong focal length on
the converging ring.  The stream case of the entry point (tests/bundle_calibration_cases.py) runs in test_gpu_streams.py.

Tolerances: ``cases.DEVICE_TOLERANCE``, ten times the spread between the oracle's Schur and dense solvers on the same
inputs (``cases.SPREAD``, measured on the CPU and re-measured by test_bundle_calibration_host.py).  Only the summation
order differs between the device and the Schur oracle, and the border sums run over all points."""
import numpy as np
import pytest
import torch

import bundle_calibration_cases as cases   # registers the stream case of the new entry point (see that module)
import bundle_calibration_oracle as bco

pytestmark = pytest.mark.gpu

TOL = cases.DEVICE_TOLERANCE


@pytest.fixture(scope="module")
def dev(native_lib):
    from structure_from_motion_amd import device

    return device.require_gpu()


def _tensors(pr):
    from structure_from_motion_amd import device

    return (device.to_device(pr["poses"]), device.to_device(pr["points"]),
            device.to_device(pr["camera_indices"], dtype=torch.int32),
            device.to_device(pr["point_indices"], dtype=torch.int32), device.to_device(pr["pixels"]))


def _run(pr, K, fixed=(0,), max_steps=50, refine=("focal",), **loss):
    """(poses, points, BundleCalibrationInfo) of the device call, and the raw tensors."""
    from structure_from_motion_amd import device

    out = device.bundle_adjust_calibrated(*_tensors(pr), K, fixed, max_steps, refine=refine, **loss)
    return out[0].cpu().numpy(), out[1].cpu().numpy(), device.read_bundle_calibration_info(out[2], out[3]), out


def _oracle(pr, K, fixed=(0,), max_steps=50, refine=("focal",), **loss):
    return bco.adjust(K, pr["poses"], pr["points"], pr["camera_indices"], pr["point_indices"], pr["pixels"], fixed, max_steps,
                      refine, **loss)


def _gaps(poses, points, info, ref):
    return dict(poses=float(np.max(np.abs(poses - ref["poses"]))), points=float(np.max(np.abs(points - ref["points"]))),
                K=float(np.max(np.abs(info.camera_matrix - ref["K"]))),
                cost=abs(info.final_cost - ref["final_cost"]) / ref["final_cost"])


def _assert_parity(name, poses, points, info, ref):
    gaps = _gaps(poses, points, info, ref)
    print(f"{name}: steps {info.steps}/{ref['steps']}, accepted {info.accepted}/{ref['accepted']}, cost "
          f"{info.initial_cost:.6g} -> {info.final_cost:.6g}, f {info.camera_matrix[0, 0]:.6f}, gaps "
          + ", ".join(f"{k} {v:.2e}" for k, v in gaps.items()))
    assert info.status == ref["status"] == 0
    assert (info.steps, info.accepted) == (ref["steps"], ref["accepted"])
    assert abs(info.initial_cost - ref["initial_cost"]) <= 1e-12 * ref["initial_cost"]
    for k, gap in gaps.items():
        assert gap <= TOL[k], (name, k, gap, TOL[k])


# ---------------------------------------------------------------------------------------------------------------------
# parity with the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.parity_cases()))
def test_parity_with_oracle(dev, name):
    """Every refine mask, two fixed cameras, the reduced system in global memory (31 free cameras), held points, both
    robust losses and a camera matrix with skew.  The test prints the measured gaps (run with -s)."""
    c = cases.parity_cases()[name]
    poses, points, info, _ = _run(c["pr"], c["K"], c["fixed"], cases.PARITY_STEPS, c["refine"], **c["loss"])
    ref = _oracle(c["pr"], c["K"], c["fixed"], cases.PARITY_STEPS, c["refine"], **c["loss"])
    _assert_parity(name, poses, points, info, ref)
    assert info.accepted >= 3 and info.final_cost < info.initial_cost
    K0, K1 = c["K"], info.camera_matrix
    assert np.array_equal(K1[2], [0.0, 0.0, 1.0])
    assert (K1[0, 1] == 0.0) == (K0[0, 1] == 0.0) and (K1[1, 0] == 0.0) == (K0[1, 0] == 0.0)   # a zero entry stays zero
    if "focal" in c["refine"]:
        # the block keeps its shape: at most five steps, each rounding K11 twice (the ratio, the product), about 1.2e-15
        assert K1[0, 0] != K0[0, 0] and abs(K1[1, 1] / K1[0, 0] - K0[1, 1] / K0[0, 0]) <= 4e-15
    else:
        assert np.array_equal(K1[:2, :2], K0[:2, :2])
    if "principal_point" in c["refine"]:
        assert K1[0, 2] != K0[0, 2] and K1[1, 2] != K0[1, 2]
    else:
        assert np.array_equal(K1[:2, 2], K0[:2, 2])
    # fixed cameras come back as they went in; held points too unless the gauge similarity of a single fixed camera moves
    # every point (then they are the oracle's, above)
    pr = c["pr"]
    moving = np.bincount(pr["point_indices"], minlength=len(pr["points"])) >= 2
    assert np.array_equal(poses[list(c["fixed"])], pr["poses"][list(c["fixed"])])
    if len(c["fixed"]) > 1:
        assert np.array_equal(points[~moving], pr["points"][~moving])
    if name == "5x60_held_points":
        assert np.count_nonzero(~moving) == 9


def test_a_point_behind_a_camera_is_a_bad_start_and_returns_the_input(dev):
    from structure_from_motion_amd import device

    c = cases.parity_cases()["3x24_all"]
    pr = dict(c["pr"], points=c["pr"]["points"].copy())
    centre = -pr["poses"][1, :9].reshape(3, 3).T @ pr["poses"][1, 9:]
    p = int(pr["point_indices"][np.nonzero(pr["camera_indices"] == 1)[0][0]])
    pr["points"][p] = centre + 2.0 * (centre - pr["points"][p])   # behind camera 1
    poses, points, info, _ = _run(pr, c["K"], refine=c["refine"])
    ref = _oracle(pr, c["K"], refine=c["refine"])
    assert info.status == ref["status"] == device.BUNDLE_BAD_START and info.steps == 0 and info.accepted == 0
    assert np.isinf(info.initial_cost) and np.isinf(info.final_cost)
    assert info.camera_matrix.tobytes() == np.ascontiguousarray(c["K"]).tobytes()
    assert np.array_equal(poses, pr["poses"]) and np.array_equal(points, pr["points"])


@pytest.mark.parametrize("which,value", [("camera_indices", 3), ("camera_indices", -1), ("point_indices", 24),
                                         ("point_indices", -1)])
def test_an_index_out_of_range_returns_the_input(dev, which, value):
    from structure_from_motion_amd import device

    c = cases.parity_cases()["3x24_all"]
    pr = dict(c["pr"])
    pr[which] = pr[which].copy()
    pr[which][5] = value
    poses, points, info, _ = _run(pr, c["K"], refine=c["refine"])
    assert info.status == device.BUNDLE_BAD_INDEX and info.steps == 0
    assert np.isnan(info.initial_cost) and np.isnan(info.final_cost)
    assert info.camera_matrix.tobytes() == np.ascontiguousarray(c["K"]).tobytes()
    assert np.array_equal(poses, pr["poses"]) and np.array_equal(points, pr["points"])


# ---------------------------------------------------------------------------------------------------------------------
# bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["32x200_global_solve", "5x60_cauchy"])
def test_two_runs_give_equal_bytes(dev, name):
    c = cases.parity_cases()[name]
    a = _run(c["pr"], c["K"], c["fixed"], 8, c["refine"], **c["loss"])[3]
    b = _run(c["pr"], c["K"], c["fixed"], 8, c["refine"], **c["loss"])[3]
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


@pytest.mark.parametrize("loss", [dict(), dict(loss="huber", loss_scale=2.0)])
def test_empty_refine_intrinsics_is_the_call_without_it(dev, loss):
    """Through the new Python argument: the same instantiations, the same bytes, the same info record."""
    from lib.bundle.bundle import bundle_adjust
    from structure_from_motion_amd import device, synthetic

    for pr, fixed in ((synthetic.bundle_problem(8, 300, seed=3), (0,)), (cases.ring_problem(32, 200, seed=13), (0, 5))):
        args = (pr["K"], pr["poses"], pr["points"], pr["camera_indices"], pr["point_indices"], pr["pixels"])
        want = bundle_adjust(*args, fixed_cameras=fixed, max_steps=10, **loss)
        got = bundle_adjust(*args, fixed_cameras=fixed, max_steps=10, refine_intrinsics=(), **loss)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        assert type(got[2]) is device.BundleInfo and got[2] == want[2] and want[2].accepted >= 3


# ---------------------------------------------------------------------------------------------------------------------
# recovery
# ---------------------------------------------------------------------------------------------------------------------
ALL = ("focal", "principal_point")


@pytest.mark.parametrize("refine", [("focal",), ALL], ids=["focal", "all"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_a_wrong_focal_length_is_recovered_on_the_ring(dev, seed, refine):
    """6 cameras x 96 points, 0.5 px noise, the focal length 5 % off, through the public API: back within 2 % of the truth
    (the oracle: 0.7 %) and equal to the oracle's; a lower cost than the same call that holds K.  The principal point is
    weakly observable there (the oracle's cy ends up to 16 px off): only device = oracle is asserted for it.  The step
    counts are printed and not asserted: each of these runs ends on an accept test of a decrease of 1e-12 of the cost or
    less (the oracle's trace), which rounding may decide either way; the runs without noise below assert them."""
    from lib.bundle.bundle import bundle_adjust

    pr = cases.ring_problem(6, 96, seed=seed)
    K = cases.wrong_camera(pr["K"], 0.05)
    args = (K, pr["poses"], pr["points"], pr["camera_indices"], pr["point_indices"], pr["pixels"])
    poses, points, info = bundle_adjust(*args, refine_intrinsics=refine)
    held = bundle_adjust(*args, refine_intrinsics=())[2]
    ref = _oracle(pr, K, refine=refine)
    focal = info.camera_matrix[0, 0]
    gaps = _gaps(poses, points, info, ref)
    print(f"seed {seed} {refine}: f {focal:.4f} (oracle {ref['K'][0, 0]:.4f}), centre {info.camera_matrix[:2, 2]}, cost "
          f"{info.final_cost:.3f} (held {held.final_cost:.3f}), steps {info.steps}/{ref['steps']}, accepted "
          f"{info.accepted}/{ref['accepted']}, gaps " + ", ".join(f"{k} {v:.2e}" for k, v in gaps.items()))
    assert info.status == 0 and abs(focal / 800.0 - 1.0) <= 0.02
    assert info.final_cost < held.final_cost
    for k, gap in gaps.items():
        assert gap <= TOL[k], (k, gap, TOL[k])


@pytest.mark.parametrize("refine", [("focal",), ALL], ids=["focal", "all"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_without_noise_the_run_is_the_oracles_to_its_last_step(dev, seed, refine):
    """Without noise every accept test is decided by most of the cost (it falls by orders of magnitude per step) and the
    run ends on the small-step stop, one step after the last accepted one: the device takes the oracle's steps, which pins
    the intrinsics' share of |delta| and |x| in that stop, and ends at the oracle's K, poses and points.  With the focal
    length alone free it comes back to cases.EXACT_FOCAL, the relative error the oracle itself ends with (8.8e-13)."""
    pr = cases.ring_problem(6, 96, seed=seed, noise_px=0.0)
    K = cases.wrong_camera(pr["K"], 0.05)
    poses, points, info, _ = _run(pr, K, refine=refine)
    ref = _oracle(pr, K, refine=refine)
    error = abs(info.camera_matrix[0, 0] / 800.0 - 1.0)
    gaps = _gaps(poses, points, info, ref)
    print(f"seed {seed} {refine}: f {info.camera_matrix[0, 0]!r}, relative error {error:.2e}, cost {info.final_cost:.2e}, "
          f"steps {info.steps}/{ref['steps']}, accepted {info.accepted}/{ref['accepted']}, gaps "
          + ", ".join(f"{k} {v:.2e}" for k, v in gaps.items() if k != "cost"))
    # the premise, on the oracle: every accept test accepted by at least 0.9 of the cost, then one step that stops
    assert min(abs(new - cur) / cur for cur, new in ref["trace"]) >= 0.9
    assert ref["steps"] == ref["accepted"] + 1 == len(ref["trace"]) + 1
    assert info.status == 0 and (info.steps, info.accepted) == (ref["steps"], ref["accepted"])
    for k in ("poses", "points", "K"):   # the final cost is 1e-20 px^2, rounding of a sum of squares: not compared
        assert gaps[k] <= TOL[k], (k, gaps[k], TOL[k])
    if refine == ("focal",):
        assert error <= cases.EXACT_FOCAL
        assert np.array_equal(info.camera_matrix[:, 2], [320.0, 240.0, 1.0])
    assert info.camera_matrix[0, 1] == 0.0 and info.camera_matrix[1, 0] == 0.0


def test_multi_view_app_shrinks_the_focal_error(dev):
    """The app with a focal length 5 % off: the final adjustment with ``--bundle-refine focal`` ends nearer the truth than
    the pipeline started."""
    from apps import sfm_multi_view

    out = sfm_multi_view.run(views=6, points=600, focal_error=0.05, bundle_refine=("focal",))
    print("focal", out["focal"], "rms_px", out["rms_px"], "registered", out["views_registered"])
    assert abs(out["focal"]["error_before"] - 0.05) < 1e-12
    assert out["views_registered"] == 6 and out["ba_status"] == 0
    assert out["focal"]["error_after"] < out["focal"]["error_before"]
