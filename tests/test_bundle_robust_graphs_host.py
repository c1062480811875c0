"""The robust losses beyond the regular graph, host side ("Tests beyond the regular graph"; no GPU):
``bundle_graphs.corrupt_long_tracks``; the robust oracle against itself under a permutation of the observations on every
parity input of tests/test_gpu_bundle_robust_graphs.py (what keeps that file's bounds honest: the reference alone must
stay a decade inside them); the loss functions against 50 digits; and the scale contract of ``sfmloss::scale_ok`` at
every door that takes a loss."""
import ctypes as C

import numpy as np
import pytest
import torch

import bundle_graphs as bg
import bundle_robust_cases as rc
import bundle_robust_oracle as bro
import geometry_cases as gc
from structure_from_motion_amd import synthetic

SFM_EINVAL = -1

# The oracle's own gap between two observation orders: the bound of every case but one_camera_case, whose V_p has rank 2
# and condition about 1 / lambda; measured there: poses 2.4e-14, points 1.2e-11 (Cauchy, 3 steps).
SELF_POSE_TOL = 1e-12
SELF_POINT_TOL = 1e-11
ONE_CAMERA_SELF_POINT_TOL = 1e-10


# ---- the helper ------------------------------------------------------------------------------------------------------------
def _multiset(pr):
    rows = np.column_stack([pr["camera_indices"], pr["point_indices"], pr["pixels"]])
    return rows[np.lexsort(rows.T[::-1])]


@pytest.mark.parametrize("name", ["dense-8", "pcg-65"])
def test_corrupt_long_tracks(name):
    _, Cn, P, seed, kw = rc.MIXED[name]
    sets = []
    for order in bg.ORDERS:
        pr = bg.mixed(Cn, P, seed, order=order, **kw)
        bad, mask = bg.corrupt_long_tracks(pr, 0.05, 200.0, 5)
        again, mask2 = bg.corrupt_long_tracks(pr, 0.05, 200.0, 5)
        assert np.array_equal(bad["pixels"], again["pixels"]) and np.array_equal(mask, mask2)
        cam, pt = pr["camera_indices"], pr["point_indices"]
        M = len(cam)
        assert mask.dtype == bool and mask.shape == (M,) and mask.sum() == int(0.05 * M) > 0
        assert np.array_equal(bad["pixels"][~mask], pr["pixels"][~mask]) and bad["pixels"] is not pr["pixels"]
        shift = bad["pixels"][mask] - pr["pixels"][mask]
        assert np.all(np.abs(shift) <= 200.0 + 1e-9) and np.max(np.abs(shift)) > 150.0
        touched = pt[mask]
        assert len(np.unique(touched)) == len(touched)   # no point twice
        for p in touched:
            assert len(np.unique(cam[pt == p])) >= 3
        for key in ("poses", "points", "camera_indices", "point_indices", "K"):
            assert bad[key] is pr[key]
        sets.append(_multiset(bad))
    for other in sets[1:]:
        assert np.array_equal(sets[0], other)   # one seed is one corrupted graph, whatever the order


def test_corrupt_long_tracks_min_cameras_and_refusal():
    pr = bg.irregular_problem(8, 1200, 12, singles=1100, unobserved=100)
    with pytest.raises(AssertionError, match="seen by at least 3"):
        bg.corrupt_long_tracks(pr, 0.05, 200.0, 5)
    bad, mask = bg.corrupt_long_tracks(pr, 0.05, 200.0, 5, min_cameras=1)
    assert mask.sum() == 55
    two = bg.irregular_problem(6, 400, 3, pairs=300)
    _, mask = bg.corrupt_long_tracks(two, 0.02, 10.0, 1)
    for p in two["point_indices"][mask]:
        assert len(np.unique(two["camera_indices"][two["point_indices"] == p])) >= 3


# ---- the oracle against itself ---------------------------------------------------------------------------------------------
def _self_gap(name, pr, pcg, point_tol=SELF_POINT_TOL, back=None, **kw):
    a = rc.oracle(pr, pcg, **kw)
    b = rc.oracle(rc.permuted(pr), pcg, **kw)
    assert a["status"] == b["status"] == 0
    assert (a["steps"], a["accepted"]) == (b["steps"], b["accepted"]), name
    if pcg:
        assert a["cg"] == b["cg"], name
    back_poses, back_points = back if back else (lambda x: x, lambda x: x)
    dp = float(np.max(np.abs(back_poses(a["poses"]) - back_poses(b["poses"]))))
    dx = float(np.max(np.abs(back_points(a["points"]) - back_points(b["points"])), initial=0.0))
    print(f"{name}: steps {a['steps']}, accepted {a['accepted']}, cg {a.get('cg')}, self gap poses {dp:.2e} points {dx:.2e}")
    assert dp <= SELF_POSE_TOL and dx <= point_tol, (name, dp, dx)
    return a, b


@pytest.mark.parametrize("loss", list(rc.LOSS))
@pytest.mark.parametrize("name", list(rc.MIXED))
def test_oracle_agrees_with_itself_on_mixed_graphs(name, loss):
    pr, mask, kw = rc.mixed_case(name, loss)
    a, _ = _self_gap(f"{name} {loss}", pr, rc.MIXED[name][0], max_steps=rc.STEPS, **kw)
    assert a["accepted"] >= 3
    assert np.mean(a["weights"] < 0.5) >= 0.03   # the case is not vacuous


def test_oracle_agrees_with_itself_at_70000_cameras():
    pr, mask, kw, fixed = rc.radix_case()
    a, _ = _self_gap("radix cauchy", pr, True, fixed=fixed, max_steps=3, **kw)
    assert a["accepted"] >= 2 and np.mean(a["weights"] < 0.5) >= 0.03


@pytest.mark.parametrize("pcg", [False, True], ids=["dense", "pcg"])
@pytest.mark.parametrize("loss", list(rc.LOSS))
def test_oracle_agrees_with_itself_on_edge_graphs(loss, pcg):
    pr, mask, kw = rc.all_held_case(loss)
    a, b = _self_gap(f"all held {loss} fixed {{0, 1}}", pr, pcg, fixed=(0, 1), max_steps=rc.STEPS, **kw)
    assert a["accepted"] >= 1
    assert np.array_equal(a["points"], pr["points"]) and np.array_equal(b["points"], pr["points"])
    _self_gap(f"all held {loss} fixed {{0}}", pr, pcg, max_steps=rc.STEPS, **kw)
    pr, mask, kw = rc.one_camera_case(loss)
    for steps in (1, 2, 3):
        a, _ = _self_gap(f"one-camera points {loss} {steps} steps", pr, pcg, point_tol=ONE_CAMERA_SELF_POINT_TOL,
                         max_steps=steps, **kw)
        assert a["accepted"] == steps
    pr, mask, kw = rc.blind_camera_case(loss)
    a = rc.oracle(pr, pcg, max_steps=50, **kw)
    assert a["status"] == 0 and a["accepted"] == 0 and a["steps"] == 20


@pytest.mark.parametrize("loss", list(rc.LOSS))
@pytest.mark.parametrize("camera", list(gc.CAMERAS))
def test_oracle_agrees_with_itself_on_cameras_and_worlds(camera, loss):
    """The gaps in the original frame and unit, as the device's are taken."""
    base, mask, kw = rc.camera_case(camera, loss)
    for world in gc.ITERATIVE_WORLDS:
        pr = gc.problem_to(world, base)
        back = (lambda x, w=world: gc.poses_back(w, x), lambda x, w=world: gc.points_back(w, x))
        for pcg in (False, True):
            a, _ = _self_gap(f"{camera}/{world} {loss} {'pcg' if pcg else 'dense'}", pr, pcg, back=back,
                             max_steps=rc.CAMERA_STEPS[loss], **kw)
            assert a["accepted"] >= 3 and np.mean(a["weights"] < 0.5) >= 0.03


@pytest.mark.parametrize("camera", ["bench", "affine", "unit"])
def test_oracle_cauchy_converges_to_one_cost_in_every_world(camera):
    """Cauchy to convergence: the same final cost in the four worlds (measured spread at most 1.5e-13 relative).  The estimates are
    not compared: the dense oracle's own point gap between two orders is 9.7e-10 by then."""
    base, mask, kw = rc.camera_case(camera, "cauchy")
    cost = {}
    for world in gc.ITERATIVE_WORLDS:
        out = rc.oracle(gc.problem_to(world, base), False, max_steps=50, **kw)
        assert out["status"] == 0 and out["steps"] < 50
        cost[world] = out["final_cost"]
    spread = max(abs(cost[w] - cost["id"]) / cost["id"] for w in cost)
    print(f"{camera}: cauchy final cost {cost['id']:.12g}, spread over the worlds {spread:.2e}")
    assert spread <= 1e-11


# ---- the losses against 50 digits ------------------------------------------------------------------------------------------
def test_rho_and_weight_against_50_digits():
    """bundle_robust_oracle.rho_and_weight (NumPy's log1p and sqrt) on the grid of the device test, e = fl(d d).  Measured
    worst error over the bound (4 * 2^-52): rho 0.136, w 0.131."""
    worst = {"rho": 0.0, "w": 0.0}
    for a in rc.RHO_SCALES:
        for loss in rc.LOSS:
            for d in rc.rho_grid(a):
                e = d * d
                f, w = bro.rho_and_weight(np.array([e]), loss, a)
                f_mp, w_mp = rc.rho_mp(e, loss, a)
                if d == 0.0:
                    assert f[0] == 0.0 and w[0] == 1.0
                worst["rho"] = max(worst["rho"], rc.relative_error(f[0], f_mp) / rc.RHO_BOUND)
                worst["w"] = max(worst["w"], rc.relative_error(w[0], w_mp) / rc.RHO_BOUND)
    print(f"rho_and_weight against 50 digits, worst error / bound: rho {worst['rho']:.3f}, w {worst['w']:.3f}")
    assert worst["rho"] <= 1.0 and worst["w"] <= 1.0
    # Huber's tie: e == a2 bit for bit takes the squared branch
    for a in rc.RHO_SCALES:
        f, w = bro.rho_and_weight(np.array([a * a]), "huber", a)
        assert f[0] == a * a and w[0] == 1.0
    # the smallest scales of the contract: a2 normal, rho tiny or +inf, never NaN
    f, _ = bro.rho_and_weight(np.array([1.0, 1e20]), "cauchy", 1e-150)
    assert rc.relative_error(f[0], rc.rho_mp(1.0, "cauchy", 1e-150)[0]) <= rc.RHO_BOUND and f[1] == np.inf
    assert 6.8e-298 < f[0] < 7.0e-298


# ---- the scale contract ----------------------------------------------------------------------------------------------------
BAD_SCALES = (1e-170, 1e-160, 5e-324, 1e155, 1e300)   # a * a is 0, subnormal, 0, inf, inf
GOOD_SCALES = (1.5e-154, 1e154)


def test_scale_rule_matches_its_definition():
    from structure_from_motion_amd import _native

    tiny = np.finfo(np.float64).tiny
    for a in BAD_SCALES + (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        assert not _native.loss_scale_ok(a), a
    for a in GOOD_SCALES + (1.0, 2.0 / 1520.0, 1e6):
        assert _native.loss_scale_ok(a) and tiny <= a * a < np.inf, a
    # outside the contract rho is NaN for every e, zero included: what the contract is for
    with np.errstate(all="ignore"):
        for a in (1e-170, 1e160):
            assert np.all(np.isnan(bro.rho_and_weight(np.array([0.0, 1.0]), "cauchy", a)[0]))


@pytest.mark.parametrize("solver", ["dense", "pcg"])
def test_bundle_entry_points_refuse_a_scale_without_a_normal_square(native_lib, solver):
    """SFM_EINVAL on the host before any launch (no GPU needed: the device pointers are never dereferenced)."""
    from structure_from_motion_amd import _native

    lib = native_lib
    Kc = (C.c_double * 9)(*[float(v) for v in synthetic.BENCH_K.reshape(9)])
    p = C.c_void_p(0x1000)
    fx = (C.c_uint8 * 4)(1, 0, 0, 0)

    def call(options, ws_bytes):
        head = (C.cast(Kc, C.c_void_p), 4, 100, 400, C.cast(fx, C.c_void_p), p, p, p, p, p, 10)
        if solver == "dense":
            return lib.sfm_bundle_adjust_ex(*head, p, p, p, p, ws_bytes, None, C.byref(options))
        return lib.sfm_bundle_adjust_pcg_ex(*head, 100, 0.1, p, p, p, p, ws_bytes, None, C.byref(options))

    for scale in BAD_SCALES:
        for loss in (0, 1, 2):
            assert call(_native.BundleOptions(loss, 0, scale), 1 << 40) == SFM_EINVAL
            assert b"options" in lib.sfm_last_error() and b"loss_scale" in lib.sfm_last_error(), (loss, scale)
            assert lib.sfm_bundle_pcg_workspace_bytes_ex(4, 100, 400, C.byref(_native.BundleOptions(loss, 0, scale))) == -1
    for scale in GOOD_SCALES:   # accepted: the call gets as far as the workspace check (still before any launch)
        for loss in (0, 1, 2):
            assert call(_native.BundleOptions(loss, 0, scale), 1000) == SFM_EINVAL
            assert b"workspace" in lib.sfm_last_error(), (loss, scale)
            assert lib.sfm_bundle_pcg_workspace_bytes_ex(4, 100, 400, C.byref(_native.BundleOptions(loss, 0, scale))) > 0


def test_averaging_entry_points_refuse_a_scale_without_a_normal_square(native_lib):
    from structure_from_motion_amd import _native

    lib = native_lib
    p = C.c_void_p(0x1000)
    err = lib.sfm_last_error
    rot = dict(loss=2, init=0, max_steps=10, max_cg_iterations=50, cg_tolerance=1e-6, step_tolerance=1e-8)
    tra = dict(rot, warmup_steps=3, reserved=0)

    def rotations(scale, ws_bytes):
        o = _native.RotavgOptions(loss_scale=scale, **rot)
        return lib.sfm_average_rotations(6, 9, p, p, p, 0, None, C.byref(o), p, p, p, p, p, p, ws_bytes, None)

    def translations(scale, ws_bytes):
        o = _native.TransavgOptions(loss_scale=scale, **tra)
        return lib.sfm_average_translations(6, 9, p, p, None, p, 0, None, C.byref(o), p, p, p, p, p, p, p, ws_bytes, None)

    for call in (rotations, translations):
        for scale in BAD_SCALES:
            assert call(scale, 1 << 40) == SFM_EINVAL and b"loss_scale" in err(), scale
        for scale in GOOD_SCALES:
            assert call(scale, 1000) == SFM_EINVAL and b"workspace too small" in err(), scale


def test_torch_ops_refuse_a_scale_without_a_normal_square(native_lib):
    from structure_from_motion_amd import ops

    op = ops.load()
    meta = dict(device="meta")
    Cn, P, M, Q = 20, 300, 1200, 130
    K = [float(v) for v in synthetic.BENCH_K.reshape(9)]
    bundle = (torch.empty((Cn, 12), dtype=torch.float64, **meta), torch.empty((P, 3), dtype=torch.float64, **meta),
              torch.empty((M,), dtype=torch.int32, **meta), torch.empty((M,), dtype=torch.int32, **meta),
              torch.empty((M, 2), dtype=torch.float64, **meta), K, [0], 50)
    pairs, w = torch.empty((Q, 2), dtype=torch.int32, **meta), torch.empty((Q,), dtype=torch.float64, **meta)
    rel, v = torch.empty((Q, 3, 3), dtype=torch.float64, **meta), torch.empty((Q, 3), dtype=torch.float64, **meta)
    calls = (lambda s: op.bundle_adjust_robust(*bundle, 2, s),
             lambda s: op.bundle_adjust_pcg_robust(*bundle, 100, 0.1, 1, s),
             lambda s: op.average_rotations(pairs, rel, w, Cn, 0, None, 2, s, 50, 500, 1e-6, 1e-8),
             lambda s: op.average_translations(pairs, v, None, w, Cn, 0, None, 1, s, 10, 500, 500, 1e-6, 1e-8))
    for call in calls:
        for scale in BAD_SCALES:
            with pytest.raises(RuntimeError, match="loss_scale"):
                call(scale)
        for scale in GOOD_SCALES:
            assert call(scale)[0].device.type == "meta"


def test_python_layers_refuse_a_scale_without_a_normal_square_before_device_work(native_lib, monkeypatch):
    from lib.bundle.bundle import bundle_adjust
    from lib.multiview.rotation_averaging import average_rotations
    from lib.multiview.translation_averaging import average_translations
    from structure_from_motion_amd import device

    def no_device(*args, **kwargs):
        raise AssertionError("device touched")

    for fn in (device.bundle_adjust, device.bundle_adjust_pcg):   # the device layer: before the op is looked up
        for scale in BAD_SCALES:
            with pytest.raises(ValueError, match="loss_scale"):
                fn(None, None, None, None, None, synthetic.BENCH_K, loss="cauchy", loss_scale=scale)
    for scale in BAD_SCALES:
        with pytest.raises(ValueError, match="loss_scale"):
            device.average_rotations(None, None, None, 3, loss="huber", loss_scale=scale)
        with pytest.raises(ValueError, match="loss_scale"):
            device.average_translations(None, None, None, 3, loss="huber", loss_scale=scale)
    monkeypatch.setattr(device, "require_gpu", no_device)
    monkeypatch.setattr(device, "to_device", no_device)
    pr = synthetic.bundle_problem(3, 20, per_point=3, seed=1)
    for solver in ("dense", "iterative"):
        for loss in ("squared", "huber", "cauchy"):
            for scale in BAD_SCALES:
                with pytest.raises(ValueError, match="loss_scale"):
                    bundle_adjust(*rc.args(pr), linear_solver=solver, loss=loss, loss_scale=scale)
            for scale in GOOD_SCALES:
                with pytest.raises(AssertionError, match="device touched"):
                    bundle_adjust(*rc.args(pr), linear_solver=solver, loss=loss, loss_scale=scale)
    from apps import sfm_multi_view

    for scale in BAD_SCALES:   # the app refuses before any work, as for a non-positive scale
        with pytest.raises(ValueError, match="bundle_loss_scale"):
            sfm_multi_view.run(bundle_loss="cauchy", bundle_loss_scale=scale)
    # the averaging solvers take degrees: the rule applies to the value the device receives (radians, or the sine)
    pairs = np.array([[0, 1], [1, 2], [2, 0]])
    rel = np.tile(np.eye(3), (3, 1, 1))
    v = np.tile(np.array([1.0, 0.0, 0.0]), (3, 1))
    for scale in BAD_SCALES[:3] + (1e-152,):   # radians(1e-152) = 1.7e-154 has a normal square, as has its sine
        refused = scale != 1e-152
        for call in (lambda s: average_rotations(3, pairs, rel, loss_scale_deg=s),
                     lambda s: average_translations(3, pairs, v, loss_scale_deg=s)):
            with pytest.raises(ValueError if refused else AssertionError, match="loss_scale_deg" if refused else "device touched"):
                call(scale)
    with pytest.raises(ValueError, match="loss_scale_deg"):
        average_rotations(3, pairs, rel, loss_scale_deg=1e156)   # 1.7e154 rad: the square overflows
    with pytest.raises(AssertionError, match="device touched"):
        average_rotations(3, pairs, rel, loss_scale_deg=1e155)
    # 1e-152 degrees pass and 8e-153 degrees (1.4e-154 rad) do not: the check is on the converted value
    with pytest.raises(ValueError, match="loss_scale_deg"):
        average_rotations(3, pairs, rel, loss_scale_deg=8e-153)
