"""Robust losses of both bundle adjusters on the MI355X (csrc/sfm_loss.h): parity with the NumPy oracle
of tests/bundle_robust_oracle.py, dense and iterative; the losses against the truth; the squared loss through the new ops
is the path without a loss, bit for bit; the edge cases of a robust call; and the multi-view app."""
import ctypes as C

import numpy as np
import pytest
import torch

import bundle_oracle as bo
import bundle_robust_oracle as bro
from structure_from_motion_amd import synthetic

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def dev(native_lib):
    from structure_from_motion_amd import device

    return device.require_gpu()


def _tensors(pr):
    from structure_from_motion_amd import device

    return (device.to_device(pr["poses"]), device.to_device(pr["points"]),
            device.to_device(pr["camera_indices"], dtype=torch.int32),
            device.to_device(pr["point_indices"], dtype=torch.int32), device.to_device(pr["pixels"]))


def _dense(pr, fixed=(0,), max_steps=50, **loss):
    from structure_from_motion_amd import device

    out = device.bundle_adjust(*_tensors(pr), pr["K"], fixed, max_steps, **loss)
    return out[0].cpu().numpy(), out[1].cpu().numpy(), device.read_bundle_info(out[2])


def _pcg(pr, fixed=(0,), max_steps=50, **loss):
    from structure_from_motion_amd import device

    out = device.bundle_adjust_pcg(*_tensors(pr), pr["K"], fixed, max_steps, **loss)
    return out[0].cpu().numpy(), out[1].cpu().numpy(), device.read_bundle_pcg_info(out[2])


def _args(pr):
    return (pr["K"], pr["poses"], pr["points"], pr["camera_indices"], pr["point_indices"], pr["pixels"])


def _corrupted(C_, P, seed, spread, per_point=4):
    pr = synthetic.bundle_problem(C_, P, per_point=per_point, seed=seed)
    bad, _ = synthetic.corrupt_observations(pr, 0.05, spread, seed=seed + 100)
    return pr, bad


def _permuted(pr):
    perm = np.random.default_rng(1).permutation(len(pr["pixels"]))
    return dict(pr, camera_indices=pr["camera_indices"][perm], point_indices=pr["point_indices"][perm],
                pixels=pr["pixels"][perm])


# ---------------------------------------------------------------------------------------------------------------------
# parity with the oracle
# ---------------------------------------------------------------------------------------------------------------------
# The tolerances of test_gpu_bundle.py::test_parity_with_oracle.  The inputs are those on which the oracle agrees with
# itself when the observations are permuted (poses <= 2e-15, points <= 4e-13, the same 10 accepted steps and CG counts):
# a point whose observations are mostly corrupted is barely held, and a parity input must not hold one.
# Ten steps: at 15 to 20 the oracle's two orders already part by an accepted step.
POSE_TOL = 1e-10
POINT_TOL = 1e-10


def _assert_parity(info, poses, points, ref, point_tol):
    assert info.status == ref["status"] == 0
    assert info.accepted == ref["accepted"] and info.accepted >= 3, (info, ref["accepted"], ref["steps"])
    assert abs(info.initial_cost - ref["initial_cost"]) <= 1e-12 * ref["initial_cost"]
    assert abs(info.final_cost - ref["final_cost"]) <= 1e-9 * ref["final_cost"], (info.final_cost, ref["final_cost"])
    assert info.final_cost < info.initial_cost
    assert np.max(np.abs(poses - ref["poses"])) <= POSE_TOL, np.max(np.abs(poses - ref["poses"]))
    assert np.max(np.abs(points - ref["points"])) <= point_tol, np.max(np.abs(points - ref["points"]))


@pytest.mark.parametrize("C_,P,seed,per_point", [(3, 200, 11, 4), (8, 2000, 12, 4), (16, 2000, 13, 4), (40, 3000, 14, 4),
                                                 (64, 2000, 15, 5)])
def test_dense_cauchy_parity_with_oracle(dev, C_, P, seed, per_point):
    """(40, 3000) and (64, 2000) have more free cameras than the LDS holds: S lives in global memory there.
    The test prints the measured gaps (run with -s)."""
    _, pr = _corrupted(C_, P, seed, 200.0, per_point)
    poses, points, info = _dense(pr, max_steps=10, loss="cauchy", loss_scale=2.0)
    ref = bro.adjust(*_args(pr), max_steps=10, loss="cauchy", loss_scale=2.0)
    print(f"dense cauchy {C_}x{P}: accepted {info.accepted}/{ref['accepted']}, cost {info.initial_cost:.6g} -> "
          f"{info.final_cost:.6g}, pose gap {np.max(np.abs(poses - ref['poses'])):.2e}, "
          f"point gap {np.max(np.abs(points - ref['points'])):.2e}")
    _assert_parity(info, poses, points, ref, POINT_TOL)


@pytest.mark.parametrize("C_,P,seed,per_point", [(16, 2000, 13, 4), (100, 3000, 14, 5)])
def test_iterative_cauchy_parity_with_oracle(dev, C_, P, seed, per_point):
    _, pr = _corrupted(C_, P, seed, 200.0, per_point)
    poses, points, info = _pcg(pr, max_steps=10, loss="cauchy", loss_scale=2.0)
    ref = bro.adjust_pcg(*_args(pr), max_steps=10, loss="cauchy", loss_scale=2.0)
    print(f"iterative cauchy {C_}x{P}: accepted {info.accepted}/{ref['accepted']}, device cg {info.cg_iterations} (max "
          f"{info.cg_max}), oracle {ref['cg']}, pose gap {np.max(np.abs(poses - ref['poses'])):.2e}, "
          f"point gap {np.max(np.abs(points - ref['points'])):.2e}")
    assert info.steps == ref["steps"]
    assert info.cg_iterations == ref["cg_iterations"] and info.cg_max == ref["cg_max"], (info, ref["cg"])
    _assert_parity(info, poses, points, ref, POINT_TOL)


@pytest.mark.parametrize("C_,P,seed", [(3, 200, 11), (8, 2000, 12), (16, 2000, 13)])
def test_dense_huber_parity_with_oracle(dev, C_, P, seed):
    """Huber at +-40 px.  A point that owns a corrupted observation keeps a constant pull of 2 a per pixel and is softer
    than the others: the oracle's own difference under a permutation of the observations is 1.3e-10 .. 6.4e-10 in the
    points there (poses <= 6e-13), so the point tolerance is 100 x that self-difference, computed here."""
    _, pr = _corrupted(C_, P, seed, 40.0)
    poses, points, info = _dense(pr, max_steps=10, loss="huber", loss_scale=2.0)
    ref = bro.adjust(*_args(pr), max_steps=10, loss="huber", loss_scale=2.0)
    other = bro.adjust(*_args(_permuted(pr)), max_steps=10, loss="huber", loss_scale=2.0)
    self_gap = float(np.max(np.abs(other["points"] - ref["points"])))
    print(f"dense huber {C_}x{P}: accepted {info.accepted}/{ref['accepted']}, oracle self gap {self_gap:.2e} (poses "
          f"{np.max(np.abs(other['poses'] - ref['poses'])):.2e}), pose gap {np.max(np.abs(poses - ref['poses'])):.2e}, "
          f"point gap {np.max(np.abs(points - ref['points'])):.2e}")
    assert other["accepted"] == ref["accepted"]
    _assert_parity(info, poses, points, ref, 100.0 * self_gap)


# ---------------------------------------------------------------------------------------------------------------------
# against the truth, on the device's output
# ---------------------------------------------------------------------------------------------------------------------
def test_device_cauchy_recovers_the_clean_result_from_gross_outliers(dev):
    """The oracle's numbers (test_bundle_robust_host.py): clean squared 4.8e-4 rad, corrupted squared 9.2e-2, Cauchy
    5.2e-4."""
    pr = synthetic.bundle_problem(16, 2000, seed=13)
    bad, _ = synthetic.corrupt_observations(pr, 0.05, 200.0, seed=113)
    clean = bro.rotation_error(_dense(pr)[0], pr["poses_true"])
    squared = bro.rotation_error(_dense(bad)[0], pr["poses_true"])
    poses, points, info = _dense(bad, loss="cauchy", loss_scale=2.0)
    cauchy = bro.rotation_error(poses, pr["poses_true"])
    print(f"clean squared {clean:.3e}  corrupted squared {squared:.3e}  cauchy {cauchy:.3e}")
    assert info.status == 0
    assert cauchy <= 2.0 * clean, (cauchy, clean)
    assert cauchy <= 0.1 * squared, (cauchy, squared)
    assert np.max(np.abs(points)) < 10.0


@pytest.mark.parametrize("C_,P,seed", [(16, 2000, 13), (8, 2000, 12), (3, 200, 11)])
def test_device_huber_halves_the_error_from_moderate_outliers(dev, C_, P, seed):
    pr, bad = _corrupted(C_, P, seed, 40.0)
    squared = bro.rotation_error(_dense(bad, max_steps=10)[0], pr["poses_true"])
    poses, points, _ = _dense(bad, max_steps=10, loss="huber", loss_scale=2.0)
    huber = bro.rotation_error(poses, pr["poses_true"])
    print(f"{C_} x {P}: squared {squared:.3e}  huber {huber:.3e}  ratio {huber / squared:.3f}")
    assert huber <= 0.5 * squared, (huber, squared)
    assert np.max(np.abs(points)) < 10.0


# ---------------------------------------------------------------------------------------------------------------------
# squared is the path without a loss
# ---------------------------------------------------------------------------------------------------------------------
def _squared_cases():
    """(name, problem, fixed, max_steps): the size of the existing determinism test and the edge cases."""
    big = synthetic.bundle_problem(16, 20000, seed=21)
    small = synthetic.bundle_problem(5, 800, seed=24)
    one = synthetic.bundle_problem(4, 300, seed=25)
    keep = one["point_indices"] != 7
    keep[np.nonzero(~keep)[0][0]] = True   # point 7 keeps one observation
    single = dict(one, camera_indices=one["camera_indices"][keep], point_indices=one["point_indices"][keep],
                  pixels=one["pixels"][keep])
    behind = one["points"].copy()
    behind[5, 2] = -3.0
    bad_pt = one["point_indices"].copy()
    bad_pt[17] = 300
    return [("16x20000", big, (0,), 50), ("max_steps=0", small, (0,), 0), ("all but one fixed", small, (0, 1, 3, 4), 50),
            ("single observation", single, (0,), 50), ("bad start", dict(one, points=behind), (0,), 50),
            ("bad index", dict(one, point_indices=bad_pt), (0,), 50)]


def _same_info(a, b):
    """Equal info records, NaN costs (BAD_INDEX) included."""
    import dataclasses

    return type(a) is type(b) and np.array_equal(dataclasses.astuple(a), dataclasses.astuple(b), equal_nan=True)


def test_squared_through_the_new_ops_is_bit_identical(dev):
    from lib.bundle.bundle import bundle_adjust
    from structure_from_motion_amd import device, ops

    op = ops.load()
    statuses = set()
    for name, pr, fixed, steps in _squared_cases():
        t = _tensors(pr)
        Kl = [float(v) for v in np.asarray(pr["K"]).reshape(9)]
        tail = (Kl, list(fixed), steps)
        want = op.bundle_adjust(*t, *tail)
        for scale in (1.0, 7.0):
            got = op.bundle_adjust_robust(*t, *tail, 0, scale)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), (name, scale)
        P_, X_ = t[0].clone(), t[1].clone()
        rec = torch.empty(4, dtype=torch.int64, device=dev)
        op.bundle_adjust_robust_(P_, X_, *t[2:], *tail, 0, 3.0, rec)
        assert torch.equal(P_, want[0]) and torch.equal(X_, want[1]) and torch.equal(rec, want[2]), name
        wantp = op.bundle_adjust_pcg(*t, *tail, 100, 0.1)
        for scale in (1.0, 7.0):
            got = op.bundle_adjust_pcg_robust(*t, *tail, 100, 0.1, 0, scale)
            assert all(torch.equal(a, b) for a, b in zip(got, wantp)), (name, scale)
        P_, X_ = t[0].clone(), t[1].clone()
        rec = torch.empty(5, dtype=torch.int64, device=dev)
        op.bundle_adjust_pcg_robust_(P_, X_, *t[2:], *tail, 100, 0.1, 0, 3.0, rec)
        assert torch.equal(P_, wantp[0]) and torch.equal(X_, wantp[1]) and torch.equal(rec, wantp[2]), name
        # the public API with loss="squared" (any scale) is the call without a loss
        info = device.read_bundle_info(want[2])
        pub = bundle_adjust(*_args(pr), fixed_cameras=fixed, max_steps=steps, loss="squared", loss_scale=7.0)
        assert np.array_equal(pub[0], want[0].cpu().numpy()) and np.array_equal(pub[1], want[1].cpu().numpy()), name
        assert _same_info(pub[2], info), name
        pubp = bundle_adjust(*_args(pr), fixed_cameras=fixed, max_steps=steps, linear_solver="iterative", loss="squared",
                             loss_scale=0.25)
        assert np.array_equal(pubp[0], wantp[0].cpu().numpy()) and np.array_equal(pubp[1], wantp[1].cpu().numpy()), name
        assert _same_info(pubp[2], device.read_bundle_pcg_info(wantp[2])), name
        statuses.add(info.status)
    assert statuses == {device.BUNDLE_OK, device.BUNDLE_BAD_START, device.BUNDLE_BAD_INDEX}


# ---------------------------------------------------------------------------------------------------------------------
# edge cases of a robust call
# ---------------------------------------------------------------------------------------------------------------------
def test_cauchy_call_is_bit_identical_across_calls(dev):
    _, pr = _corrupted(16, 20000, 21, 200.0)
    for run in (_dense, _pcg):
        a = run(pr, max_steps=10, loss="cauchy", loss_scale=2.0)
        b = run(pr, max_steps=10, loss="cauchy", loss_scale=2.0)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
        assert a[2].accepted >= 3


@pytest.mark.parametrize("loss", ["huber", "cauchy"])
def test_point_behind_a_camera_is_a_bad_start(dev, loss):
    from structure_from_motion_amd import device

    pr = synthetic.bundle_problem(4, 300, seed=26)
    behind = pr["points"].copy()
    behind[5, 2] = -3.0
    for run in (_dense, _pcg):
        poses, points, info = run(dict(pr, points=behind), loss=loss, loss_scale=2.0)
        assert info.status == device.BUNDLE_BAD_START and info.steps == 0 and np.isinf(info.initial_cost)
        assert np.array_equal(poses, pr["poses"]) and np.array_equal(points, behind)
    bad_cam = pr["camera_indices"].copy()
    bad_cam[17] = -1
    for run in (_dense, _pcg):
        poses, points, info = run(dict(pr, camera_indices=bad_cam), loss=loss, loss_scale=2.0)
        assert info.status == device.BUNDLE_BAD_INDEX and np.isnan(info.initial_cost)
        assert np.array_equal(poses, pr["poses"]) and np.array_equal(points, pr["points"])


@pytest.mark.parametrize("loss", ["huber", "cauchy"])
def test_fixed_cameras_and_the_gauge_distance_are_kept(dev, loss):
    _, pr = _corrupted(6, 1000, 22, 40.0)
    for run in (_dense, _pcg):
        poses, _, info = run(pr, fixed=(2,), loss=loss, loss_scale=2.0)
        assert info.accepted >= 1
        assert np.array_equal(poses[2], pr["poses"][2])
        c0 = bo.centre(pr["poses"][2])
        before = np.linalg.norm(bo.centre(pr["poses"][0]) - c0)
        assert abs(np.linalg.norm(bo.centre(poses[0]) - c0) - before) <= 1e-12 * before
        poses, _, info = run(pr, fixed=(0, 1, 3, 4), loss=loss, loss_scale=2.0)
        assert info.accepted >= 1 and not np.array_equal(poses[2], pr["poses"][2])
        for c in (0, 1, 3, 4):
            assert np.array_equal(poses[c], pr["poses"][c])


def test_huge_scale_huber_equals_squared(dev):
    """loss_scale = 1e6: every e <= a^2, so w = 1, x * 1.0 is exact and rho = e: Huber equals squared bit for bit.

    Cauchy is only close: its w is never exactly 1 (1 / (1 + e / 1e12) rounds to 1 only below e = 1e-4).  The largest e
    here is (200 sqrt 2)^2 = 8e4 px^2, so w and rho / e differ from 1 by at most e / a^2 = 8e-8: that bounds the cost at a
    given estimate (1e-6 leaves an order of magnitude), but not the estimate, since a point that owns a +-200 px
    observation is held weakly along its depth under the squared loss and the perturbation of its weight is amplified by
    that conditioning.  How far the estimate moves is therefore taken from the reference: the oracle's own gap between
    its Cauchy (1e6) and its squared run, computed here (dense: poses 1.9e-9, points 8.58e-6; iterative: 2.3e-9 and
    7.32e-6).  The device measures the same quantity and may differ from it by rounding only; twice the oracle's gap
    is the bound.  Measured on the device, dense: points 8.58e-6."""
    _, pr = _corrupted(8, 2000, 12, 200.0)
    for run, oracle in ((_dense, bro.adjust), (_pcg, bro.adjust_pcg)):
        sq = run(pr, max_steps=10)
        hu = run(pr, max_steps=10, loss="huber", loss_scale=1e6)
        assert np.array_equal(hu[0], sq[0]) and np.array_equal(hu[1], sq[1]) and hu[2] == sq[2]
        ca = run(pr, max_steps=10, loss="cauchy", loss_scale=1e6)
        ref_sq = oracle(*_args(pr), max_steps=10)
        ref_ca = oracle(*_args(pr), max_steps=10, loss="cauchy", loss_scale=1e6)
        pose_gap = float(np.max(np.abs(ref_ca["poses"] - ref_sq["poses"])))
        point_gap = float(np.max(np.abs(ref_ca["points"] - ref_sq["points"])))
        print(f"{run.__name__}: cauchy 1e6 against squared, oracle poses {pose_gap:.2e} points {point_gap:.2e}; device "
              f"poses {np.max(np.abs(ca[0] - sq[0])):.2e} points {np.max(np.abs(ca[1] - sq[1])):.2e}")
        assert ca[2].accepted == sq[2].accepted == ref_ca["accepted"] == ref_sq["accepted"]
        assert abs(ca[2].final_cost - sq[2].final_cost) <= 1e-6 * sq[2].final_cost
        assert not np.array_equal(ca[0], sq[0])
        assert np.max(np.abs(ca[0] - sq[0])) <= 2.0 * pose_gap, (np.max(np.abs(ca[0] - sq[0])), pose_gap)
        assert np.max(np.abs(ca[1] - sq[1])) <= 2.0 * point_gap, (np.max(np.abs(ca[1] - sq[1])), point_gap)


def test_robust_inplace_ops_match_functional(dev):
    from structure_from_motion_amd import device

    _, pr = _corrupted(5, 1000, 27, 200.0)
    t = _tensors(pr)
    for fn, words, read in ((device.bundle_adjust, 4, device.read_bundle_info),
                            (device.bundle_adjust_pcg, 5, device.read_bundle_pcg_info)):
        want = fn(*t, pr["K"], loss="cauchy", loss_scale=2.0)
        P_, X_ = t[0].clone(), t[1].clone()
        rec = torch.empty(words, dtype=torch.int64, device=dev)
        fn(None, None, *t[2:], pr["K"], out=(P_, X_, rec), loss="cauchy", loss_scale=2.0)
        assert torch.equal(P_, want[0]) and torch.equal(X_, want[1]) and torch.equal(rec, want[2])
        assert read(rec).accepted >= 3
        plain = fn(*t, pr["K"])
        assert not torch.equal(plain[0], want[0])   # the loss took effect


def test_public_api_matches_device_with_a_loss(dev):
    from lib.bundle.bundle import bundle_adjust

    _, pr = _corrupted(4, 400, 28, 200.0)
    poses, points, info = bundle_adjust(*_args(pr), max_steps=30, loss="cauchy", loss_scale=2.0)
    ref = _dense(pr, max_steps=30, loss="cauchy", loss_scale=2.0)
    assert np.array_equal(poses, ref[0]) and np.array_equal(points, ref[1]) and info == ref[2]
    poses, points, info = bundle_adjust(*_args(pr), max_steps=30, linear_solver="iterative", loss="huber", loss_scale=3.0)
    ref = _pcg(pr, max_steps=30, loss="huber", loss_scale=3.0)
    assert np.array_equal(poses, ref[0]) and np.array_equal(points, ref[1]) and info == ref[2]


def test_c_entry_points_refuse_bad_options_on_real_buffers(dev, native_lib):
    """SFM_EINVAL with device buffers that a good call accepts: nothing is launched and the outputs keep their bytes."""
    from structure_from_motion_amd import _native

    pr = synthetic.bundle_problem(4, 300, seed=29)
    t = _tensors(pr)
    Cn, P, M = 4, 300, len(pr["pixels"])
    Kc = (C.c_double * 9)(*[float(v) for v in np.asarray(pr["K"]).reshape(9)])
    fx = (C.c_uint8 * 4)(1, 0, 0, 0)
    poses_out = torch.full_like(t[0], -7.0)
    points_out = torch.full_like(t[1], -7.0)
    info = torch.zeros(5, dtype=torch.int64, device=dev)
    bytes_ = native_lib.sfm_bundle_pcg_workspace_bytes_ex(Cn, P, M, C.byref(_native.BundleOptions(2, 0, 2.0)))
    ws = torch.empty(max(bytes_, native_lib.sfm_bundle_workspace_bytes(Cn, P, M)), dtype=torch.uint8, device=dev)
    head = (C.cast(Kc, C.c_void_p), Cn, P, M, C.cast(fx, C.c_void_p), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(),
            t[3].data_ptr(), t[4].data_ptr(), 5)
    tail = (poses_out.data_ptr(), points_out.data_ptr(), info.data_ptr(), ws.data_ptr(), ws.numel(), None)
    for bad in (_native.BundleOptions(3, 0, 2.0), _native.BundleOptions(1, 1, 2.0), _native.BundleOptions(2, 0, 0.0),
                _native.BundleOptions(2, 0, -1.0)):
        assert native_lib.sfm_bundle_adjust_ex(*head, *tail, C.byref(bad)) == -1
        assert native_lib.sfm_bundle_adjust_pcg_ex(*head, 100, 0.1, *tail, C.byref(bad)) == -1
    torch.cuda.synchronize()
    assert bool((poses_out == -7.0).all()) and bool((points_out == -7.0).all())
    # and a good call through the same buffers runs
    good = _native.BundleOptions(2, 0, 2.0)
    assert native_lib.sfm_bundle_adjust_pcg_ex(*head, 100, 0.1, *tail, C.byref(good)) == _native.SFM_OK
    torch.cuda.synchronize()
    from structure_from_motion_amd import device

    want = device.bundle_adjust_pcg(*t, pr["K"], max_steps=5, loss="cauchy", loss_scale=2.0)
    assert torch.equal(poses_out, want[0]) and torch.equal(points_out, want[1]) and torch.equal(info, want[2])


# ---------------------------------------------------------------------------------------------------------------------
# the multi-view app
# ---------------------------------------------------------------------------------------------------------------------
def _worst(out):
    return max(out["rotation_error_rad"].values()), max(out["translation_error"].values())


def test_app_squared_is_the_default_run_and_never_reaches_the_new_ops(dev, monkeypatch):
    from apps import sfm_multi_view
    from structure_from_motion_amd import ops

    op = ops.load()

    def refuse(*args, **kwargs):
        raise AssertionError("a squared run reached a robust op")

    for name in ("bundle_adjust_robust", "bundle_adjust_robust_", "bundle_adjust_pcg_robust", "bundle_adjust_pcg_robust_"):
        getattr(op, name)   # resolve the real op first, so that monkeypatch restores it
        monkeypatch.setattr(op, name, refuse)
    default = sfm_multi_view.run()
    squared = sfm_multi_view.run(bundle_loss="squared", bundle_loss_scale=7.0)
    assert default.keys() == squared.keys()
    for key in default:
        assert default[key] == squared[key], key
    with pytest.raises(AssertionError, match="robust op"):
        sfm_multi_view.run(bundle_loss="cauchy")


@pytest.mark.parametrize("tracks", ["given", "matches"])
def test_app_with_cauchy_registers_every_view_within_the_app_margin(dev, tracks):
    """The project's app margin (test_gpu_p3p.py, test_gpu_track_build.py): the largest rotation error may exceed the
    squared run's by 2e-3 rad, the largest translation error by 2e-2.  The test prints both runs' numbers (run with -s)."""
    from apps import sfm_multi_view

    squared = sfm_multi_view.run(tracks=tracks)
    cauchy = sfm_multi_view.run(tracks=tracks, bundle_loss="cauchy")
    (rs, ts), (rc, tc) = _worst(squared), _worst(cauchy)
    print(f"tracks={tracks}: squared rot {rs:.3e} trans {ts:.3e} rms {squared['rms_px']:.4f} points {squared['points_ok']}"
          f" | cauchy rot {rc:.3e} trans {tc:.3e} rms {cauchy['rms_px']:.4f} points {cauchy['points_ok']}")
    assert cauchy["views_registered"] == 8 and cauchy["ba_status"] == 0
    assert rc <= rs + 2e-3, (rc, rs)
    assert tc <= ts + 2e-2, (tc, ts)
    assert np.isfinite(cauchy["rms_px"]) and cauchy["rms_px"] > 0.0
