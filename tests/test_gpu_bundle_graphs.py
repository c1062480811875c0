"""Bundle adjustment and track triangulation on irregular observation graphs (tests/bundle_graphs.py) on the MI355X: mixed
track lengths, duplicated observations, held and unobserved points, sparse cameras, interleaved fixed sets and the four
observation orders, against the NumPy oracles of tests/bundle_oracle.py, tests/bundle_pcg_oracle.py and
tests/tracks_oracle.py.  The shapes are chosen to reach the code that uniform graphs leave alone: the merge-join of
bundle_schur_kernel over repeated points, the held-point tests, per-camera chunks of few observations, the slots of
interleaved fixed sets, both homes of the dense solve (F = 30 in LDS, F = 31 in global memory, at C = 31, 32 and 64), the
camera order's three radix passes (C = 70 000), the CG chunk of 10 and the point order's second scan level (P > 4 194 304)."""
import math

import numpy as np
import pytest
import torch

import bundle_graphs as bg
import bundle_oracle as bo
import bundle_pcg_oracle as pco
import tracks_oracle as to

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(native_lib):
    from structure_from_motion_amd import device

    return device.require_gpu()


def _dense(pr, fixed=(0,), max_steps=50):
    from structure_from_motion_amd import device

    out = device.bundle_adjust(device.to_device(pr["poses"]), device.to_device(pr["points"]),
                               device.to_device(pr["camera_indices"], dtype=torch.int32),
                               device.to_device(pr["point_indices"], dtype=torch.int32), device.to_device(pr["pixels"]),
                               pr["K"], fixed, max_steps)
    return out[0].cpu().numpy(), out[1].cpu().numpy(), device.read_bundle_info(out[2])


def _pcg(pr, fixed=(0,), max_steps=50, max_cg_iterations=100, cg_tolerance=0.1):
    from structure_from_motion_amd import device

    out = device.bundle_adjust_pcg(device.to_device(pr["poses"]), device.to_device(pr["points"]),
                                   device.to_device(pr["camera_indices"], dtype=torch.int32),
                                   device.to_device(pr["point_indices"], dtype=torch.int32), device.to_device(pr["pixels"]),
                                   pr["K"], fixed, max_steps, max_cg_iterations, cg_tolerance)
    return out[0].cpu().numpy(), out[1].cpu().numpy(), device.read_bundle_pcg_info(out[2])


def _oracle(pr, **kw):
    return bo.adjust(pr["K"], pr["poses"], pr["points"], pr["camera_indices"], pr["point_indices"], pr["pixels"], **kw)


def _oracle_pcg(pr, **kw):
    return pco.adjust_pcg(pr["K"], pr["poses"], pr["points"], pr["camera_indices"], pr["point_indices"], pr["pixels"], **kw)


def _check(name, got, ref, pose_tol, point_tol):
    """The parity assertions of tests/test_gpu_bundle.py and tests/test_gpu_bundle_pcg.py."""
    poses, points, info = got
    dp, dx = np.max(np.abs(poses - ref["poses"]), initial=0.0), np.max(np.abs(points - ref["points"]), initial=0.0)
    print(f"{name}: steps {info.steps}, accepted {info.accepted}, pose gap {dp:.2e}, point gap {dx:.2e}")
    assert info.status == ref["status"]
    assert info.steps == ref["steps"] and info.accepted == ref["accepted"], (info, ref["steps"], ref["accepted"])
    if "cg" in ref:
        assert info.cg_iterations == ref["cg_iterations"] and info.cg_max == ref["cg_max"], (info, ref["cg"])
    assert abs(info.initial_cost - ref["initial_cost"]) <= 1e-12 * ref["initial_cost"]
    assert abs(info.final_cost - ref["final_cost"]) <= 1e-9 * ref["final_cost"], (info.final_cost, ref["final_cost"])
    assert dp <= pose_tol and dx <= point_tol, (dp, dx)


# Tolerances, calibrated on the CPU by running the oracle on each graph in two observation orders (random and
# camera-major; only the summation order changes, as between the device and the oracle).  Measured gaps:
#   dense mixed 8 / 31 / 32 x 3 000 to convergence (6-7 steps): poses 1.6e-15, points 1.2e-13;
#   dense mixed 64 x 3 000, fixed {0}, to convergence (11 steps): poses 2.4e-15, points 1.4e-13;
#   PCG mixed 65 x 4 000 and 300 x 20 000 to convergence (8-9 steps): poses 2.5e-15, points 5.2e-13;
#   PCG at the CG caps 1 .. 21, 3 steps: poses 4.5e-15, points 8.5e-12 (CG stopped short leaves the points less settled);
#   all points held (4 steps): poses 8.3e-16, points 6.2e-15;
#   one-camera moving points, 1 .. 3 steps: poses 9.6e-15, points 4.9e-13.
# 1e-10 is the bound of the existing parity tests; it keeps more than an order of margin over the worst of these.
POSE_TOL = 1e-10
POINT_TOL = 1e-10
# The C = 64 fixed sets other than {0} hold perturbed cameras fixed, so the fit is inconsistent and a few two-view points
# run off along their nearly parallel rays: the graph is ill-conditioned along its path and the gap grows with the steps
# (even cameras: points 3.5e-12 after 3 steps, 4.2e-11 after 4, 1.2e-10 after 5; {63}: 1.2e-9 after 8, 2.4e-5 after 12;
# {0 .. 33}: 3.5e-5 after 8).  These cases therefore run 3 steps, where the worst gaps over the five sets are poses
# 1.3e-14 and points 4.7e-12.  A permutation of the observations cannot show the rounding of a two-view point, whose
# sums of two terms do not depend on their order; on the device the all-but-one set, whose only free camera is the sparse
# one, measured points 1.6e-10 (poses 2.6e-16), the rest at most 9.5e-12.  FIXED_POINT_TOL keeps 60 times that.
FIXED_STEPS = 3
FIXED_POINT_TOL = 1e-8


# ------------------------------------------------------------------------------------------------------------------------
# Dense path
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["random", "camera-major"])
@pytest.mark.parametrize("C,P,seed", [(8, 3000, 1), (31, 3000, 2), (32, 3000, 3), (64, 3000, 4)])
def test_dense_mixed_graph_parity(dev, C, P, seed, order):
    """C = 31: F = 30, S in LDS; C = 32: F = 31, S in global memory.  Full-length tracks only at C <= 32 (the Schur oracle
    costs the square of the longest track)."""
    pr = bg.mixed(C, P, seed, order=order, full=C <= 32)
    got = _dense(pr)
    ref = _oracle(pr)
    assert ref["status"] == 0 and ref["accepted"] >= 3
    _check(f"dense {C} x {P} {order}", got, ref, POSE_TOL, POINT_TOL)


@pytest.mark.parametrize("fixed", [(63,), (5,), tuple(range(34)), tuple(range(0, 64, 2)),
                                   tuple(c for c in range(64) if c != 17)],
                         ids=["63", "5", "0-33", "even", "all-but-17"])
def test_dense_fixed_sets_at_64_cameras(dev, fixed):
    """{63}: the mask's top bit, gauge anchor camera 0; {0 .. 33}: F = 30 takes the LDS path at C = 64; the even cameras:
    F = 32 with interleaved slots.  The sparse camera (10 observations) is free in every set."""
    pr = bg.mixed(64, 3000, 7, order="camera-major", full=False, sparse_camera=17 if len(fixed) == 63 else 61)
    got = _dense(pr, fixed=fixed, max_steps=FIXED_STEPS)
    ref = _oracle(pr, fixed=fixed, max_steps=FIXED_STEPS)
    assert ref["status"] == 0 and ref["accepted"] >= 2
    _check(f"dense 64 fixed {len(fixed)}", got, ref, POSE_TOL, FIXED_POINT_TOL)
    for c in fixed:
        assert np.array_equal(got[0][c], pr["poses"][c])


def _edge(pr, fixed, max_steps):
    got = _dense(pr, fixed=fixed, max_steps=max_steps)
    ref = _oracle(pr, fixed=fixed, max_steps=max_steps)
    poses, points, info = got
    assert (info.status, info.steps, info.accepted) == (ref["status"], ref["steps"], ref["accepted"]), (info, ref)
    assert abs(info.initial_cost - ref["initial_cost"]) <= 1e-12 * ref["initial_cost"]
    if ref["accepted"] == 0:
        assert info.final_cost == info.initial_cost
        assert np.array_equal(poses, pr["poses"]) and np.array_equal(points, pr["points"])
    return got, ref


def test_dense_free_camera_without_observations_rejects_every_step(dev):
    """U_c = 0 for the free camera that sees nothing: S does not factor, every step is rejected until lambda passes 1e16
    (20 steps), and the input comes back bit-unchanged."""
    pr = bg.mixed(8, 1000, 11, sparse_count=0)
    got, ref = _edge(pr, (0,), 50)
    assert ref["accepted"] == 0 and ref["steps"] == 20


def test_dense_every_point_held(dev):
    """Every point seen once: nothing is moving, S = U*, only the cameras move.  With two fixed cameras the points are
    bit-unchanged; with one, the gauge rescale moves them as in the oracle."""
    pr = bg.irregular_problem(8, 1200, 12, singles=1100, unobserved=100)
    got, ref = _edge(pr, (0, 1), 20)
    assert ref["accepted"] >= 1
    assert np.array_equal(got[1], pr["points"])
    _check("dense all held, fixed {0, 1}", got, ref, POSE_TOL, POINT_TOL)
    got = _dense(pr, max_steps=20)
    _check("dense all held, fixed {0}", got, _oracle(pr, max_steps=20), POSE_TOL, POINT_TOL)


@pytest.mark.parametrize("P", [10, 0])
def test_dense_no_observations(dev, P):
    """M = 0 (with points, and with none): the cost is 0, S = 0 does not factor, 20 rejected steps, input unchanged."""
    pr = bg.irregular_problem(4, P, 13, unobserved=P)
    assert len(pr["camera_indices"]) == 0
    got, ref = _edge(pr, (0,), 50)
    assert ref["initial_cost"] == got[2].initial_cost == 0.0 and ref["steps"] == 20


@pytest.mark.parametrize("max_steps", [1, 2, 3])
def test_dense_one_camera_moving_points(dev, max_steps):
    """Points seen twice by one camera are moving points whose V_p has rank 2: V_p* still factors (its pivots are positive)
    and is inverted as it stands.  Their depth is ill-conditioned (condition about 1 / lambda), so the gap
    grows with the steps as lambda falls: measured on the CPU in two orders, points 4.9e-13 after 3 steps and 3.8e-11
    after 6.  These cases run at most 3 steps."""
    pr = bg.mixed(8, 3000, 14, one_camera=20)
    got, ref = _edge(pr, (0,), max_steps)
    assert ref["accepted"] == max_steps
    _check(f"dense one-camera points, {max_steps} steps", got, ref, POSE_TOL, POINT_TOL)


# ------------------------------------------------------------------------------------------------------------------------
# Iterative path
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["random", "camera-major"])
@pytest.mark.parametrize("C,P,seed", [(65, 4000, 21), (300, 20000, 22)])
def test_pcg_mixed_graph_parity(dev, C, P, seed, order):
    """Full-length tracks of C - 1 views (the PCG oracle is matrix-free), duplicates, held, unobserved and one sparse free
    camera."""
    pr = bg.mixed(C, P, seed, order=order)
    got = _pcg(pr)
    ref = _oracle_pcg(pr)
    assert ref["status"] == 0 and ref["accepted"] >= 3
    _check(f"pcg {C} x {P} {order}", got, ref, POSE_TOL, POINT_TOL)


def test_pcg_radix_order_at_70000_cameras(dev):
    """C = 70 000 (three 8-bit radix passes) and about 200 000 observations over every camera, in camera-major order so
    that one digit fills whole tiles and waves.  The free cameras share low bytes (1, 257, 513, 65 537, 65 793: equal in
    the first byte; 69 999 the last camera) plus 20 more; each sees exactly 40 points.  Everything else is fixed."""
    C = 70000
    rng = np.random.default_rng(31)
    free = [1, 257, 513, 65537, 65793, 69999] + sorted(rng.choice(np.arange(2, 69999), 20, replace=False).tolist())
    pr = bg.irregular_problem(C, 70000, 31, singles=5000, pairs=15000, mid=(3, 4), duplicates=1000,
                              sparse={c: 40 for c in free}, order="camera-major")
    assert 190000 <= len(pr["camera_indices"]) <= 230000
    assert len(np.unique(pr["camera_indices"])) >= 0.9 * C   # about 3 observations per camera: a few see none
    fixed = np.setdiff1d(np.arange(C), free).tolist()
    got = _pcg(pr, fixed=fixed, max_steps=3)
    ref = _oracle_pcg(pr, fixed=fixed, max_steps=3)
    assert ref["status"] == 0 and ref["accepted"] >= 2
    _check("pcg 70 000 cameras", got, ref, POSE_TOL, POINT_TOL)
    assert np.array_equal(got[0][fixed], pr["poses"][fixed])


@pytest.mark.parametrize("cap", [1, 9, 10, 11, 21])
def test_pcg_cg_chunk_boundaries(dev, cap):
    """cg_tolerance 1e-30 (0 is refused): every step runs CG to the cap, which lands on both sides of the host's chunk of
    10 iterations."""
    pr = bg.mixed(65, 4000, 23)
    got = _pcg(pr, max_steps=3, max_cg_iterations=cap, cg_tolerance=1e-30)
    ref = _oracle_pcg(pr, max_steps=3, max_cg_iterations=cap, cg_tolerance=1e-30)
    assert ref["cg"] == [cap] * ref["steps"]
    _check(f"pcg cap {cap}", got, ref, POSE_TOL, POINT_TOL)


# ------------------------------------------------------------------------------------------------------------------------
# Track triangulation over the same graphs, and the point order past 1 024 scan tiles
# ------------------------------------------------------------------------------------------------------------------------
K = bg.synthetic.BENCH_K
MIN_ANGLE = np.radians(1.0)
MAX_ERROR = 16.0
# The bounds and the status band of tests/test_gpu_tracks.py (linear: POINT_TOL, VALUE_TOL; refined: REFINED_POINT_TOL,
# REFINED_ERROR_TOL, COST_TOL).
TRACK_POINT_TOL = 1e-9
TRACK_VALUE_TOL = 1e-9
REFINED_POINT_TOL = 1e-6
REFINED_ERROR_TOL = 1e-5
COST_TOL = 1e-9
STATUS_BAND = 1e-6


def _tracks(poses, cam, pt, uv, P, refine):
    from structure_from_motion_amd import device

    X, status, err, angle, info = device.triangulate_tracks(
        device.to_device(poses), device.to_device(cam, dtype=torch.int32), device.to_device(pt, dtype=torch.int32),
        device.to_device(uv), P, K, 2, MIN_ANGLE, MAX_ERROR, refine)
    return dict(points=X.cpu().numpy(), status=status.cpu().numpy(), obs_error=err.cpu().numpy(), angle=angle.cpu().numpy(),
                info=device.read_tracks_info(info))


def _compare_tracks(name, got, ref, pt, P, refine):
    """tests/test_gpu_tracks.py's parity assertions over the points 0 .. P - 1 of (pt, ref)."""
    max_e = np.full(P, np.nan)
    ok_e = ~np.isnan(ref["obs_error"])
    np.fmax.at(max_e, pt[ok_e], ref["obs_error"][ok_e])
    near = (np.abs(ref["angle"] - MIN_ANGLE) <= STATUS_BAND * MIN_ANGLE) | \
           (np.abs(max_e - MAX_ERROR) <= STATUS_BAND * MAX_ERROR)
    differ = got["status"] != ref["status"]
    assert not np.any(differ & ~near), np.nonzero(differ & ~near)[0][:10]
    assert np.count_nonzero(differ) <= max(2, P // 1000)
    same = ~differ
    assert np.array_equal(np.isnan(got["points"][same]), np.isnan(ref["points"][same]))
    wide = same & (ref["angle"] >= MIN_ANGLE)
    scale = np.linalg.norm(ref["points"][wide], axis=1)
    dp = np.max(np.abs(got["points"][wide] - ref["points"][wide]), axis=1) / scale
    da = np.abs(got["angle"][wide] - ref["angle"][wide])
    obs = wide[pt] & np.isfinite(ref["obs_error"])
    de = np.abs(got["obs_error"][obs] - ref["obs_error"][obs]) / np.maximum(1.0, np.abs(ref["obs_error"][obs]))
    cost_got = np.bincount(pt[obs], weights=got["obs_error"][obs], minlength=P)[wide]
    cost_ref = np.bincount(pt[obs], weights=ref["obs_error"][obs], minlength=P)[wide]
    dc = np.abs(cost_got - cost_ref) / np.maximum(1.0, cost_ref)
    print(f"{name} refine={refine}: points {dp.max():.3g}, angle {da.max():.3g}, error {de.max():.3g}, "
          f"point cost {dc.max():.3g}, status differences {np.count_nonzero(differ)}")
    if refine == 0:
        assert dp.max() <= TRACK_POINT_TOL and da.max() <= TRACK_VALUE_TOL and de.max() <= TRACK_VALUE_TOL
    else:
        assert dp.max() <= REFINED_POINT_TOL and da.max() <= REFINED_POINT_TOL and de.max() <= REFINED_ERROR_TOL
    assert dc.max() <= COST_TOL
    assert np.array_equal(np.isnan(got["obs_error"]), np.isnan(ref["obs_error"]))
    assert np.array_equal(np.isinf(got["obs_error"]), np.isinf(ref["obs_error"]))


@pytest.mark.parametrize("refine", [0, 10])
@pytest.mark.parametrize("order", bg.ORDERS)
@pytest.mark.parametrize("C,P,seed", [(8, 3000, 41), (64, 5000, 42)])
def test_tracks_mixed_graph_orders(dev, C, P, seed, order, refine):
    """Mixed track lengths with 8- and 64-view tracks, duplicates, single-view and unobserved points, in every order."""
    pr = bg.irregular_problem(C, P, seed, singles=P // 10, unobserved=P // 50, pairs=P // 5, full=5,
                              duplicates=P // 20, order=order)
    cam, pt, uv = pr["camera_indices"], pr["point_indices"], pr["pixels"]
    got = _tracks(pr["poses_true"], cam, pt, uv, P, refine)
    ref = to.triangulate(K, pr["poses_true"], cam, pt, uv, P, min_angle=MIN_ANGLE, max_error=MAX_ERROR,
                         refine_steps=refine)
    assert got["info"].status == 0
    assert got["info"].points_ok == np.count_nonzero(got["status"] == to.OK)
    if refine:
        assert got["info"].max_refine_steps_taken == ref["info"]["max_refine_steps_taken"]
    _compare_tracks(f"tracks {C} x {P} {order}", got, ref, pt, P, refine)


BIG_P = 4_200_000   # the point order's scan runs over 4 096-entry tiles: more than 1 024 of them


@pytest.fixture(scope="module")
def big_graph():
    """16 cameras, 4.2 M points with 2 or 3 observations each (10.5 M observations), camera-major."""
    return bg.irregular_problem(16, BIG_P, 43, pairs=BIG_P // 2, mid=(3, 3), order="camera-major")


@pytest.mark.parametrize("refine", [0, 10])
def test_tracks_past_1024_scan_tiles(dev, big_graph, refine):
    """Tracks are independent per point, so the oracle runs on a fixed sample of 100 000 points and their observations;
    over all points the device's status counts add up to P."""
    pr = big_graph
    cam, pt, uv = pr["camera_indices"], pr["point_indices"], pr["pixels"]
    got = _tracks(pr["poses_true"], cam, pt, uv, BIG_P, refine)
    assert got["info"].status == 0
    counts = np.bincount(got["status"], minlength=7)
    assert counts.sum() == BIG_P and counts[to.FEW_VIEWS] == 0 and counts[to.BAD_INDEX] == 0
    assert got["info"].points_ok == counts[to.OK]
    sample = np.sort(np.random.default_rng(44).choice(BIG_P, 100_000, replace=False))
    keep = np.isin(pt, sample)
    remap = np.full(BIG_P, -1)
    remap[sample] = np.arange(len(sample))
    spt = remap[pt[keep]]
    ref = to.triangulate(K, pr["poses_true"], cam[keep], spt, uv[keep], len(sample), min_angle=MIN_ANGLE,
                         max_error=MAX_ERROR, refine_steps=refine)
    sub = dict(points=got["points"][sample], status=got["status"][sample], obs_error=got["obs_error"][keep],
               angle=got["angle"][sample])
    _compare_tracks("tracks 16 x 4.2 M sample", sub, ref, spt, len(sample), refine)


def test_dense_initial_cost_past_1024_scan_tiles(dev, big_graph):
    """max_steps = 0 over the 4.2 M-point graph: the device's starting cost is math.fsum of the oracle's e to 1e-12."""
    pr = big_graph
    poses, points, info = _dense(pr, max_steps=0)
    M = len(pr["camera_indices"])
    e = [bo.residuals(pr["poses"], pr["points"], pr["camera_indices"][s:s + (1 << 20)], pr["point_indices"][s:s + (1 << 20)],
                      pr["pixels"][s:s + (1 << 20)], pr["K"])[0] for s in range(0, M, 1 << 20)]
    total = math.fsum(np.concatenate(e))
    assert info.status == 0 and info.steps == 0 and info.accepted == 0
    assert abs(info.initial_cost - total) <= 1e-12 * total, (info.initial_cost, total)
    assert info.final_cost == info.initial_cost
    assert np.array_equal(poses, pr["poses"]) and np.array_equal(points, pr["points"])
