"""Host side of the pose entry of the view-graph call: the exports, the argument checks of ``sfm_pair_poses``
and of ``verify_pairs``, the NumPy definition against the truth of noise-free scenes, the angle gate of ``choose_seed_pair``
and the condition the GPU tests' exact vote comparison rests on.  Nothing here needs a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import view_graph_oracle as vo
import view_graph_pose_oracle as po
from structure_from_motion_amd.epipolar import view_graph as vg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = vo.ho.synthetic.BENCH_K
EINVAL = -1   # SFM_EINVAL


def test_exports_and_op_schema(native_lib):
    from structure_from_motion_amd import _native, build, device, ops

    assert "sfm_view_graph_pose.hip" in build.SOURCES
    assert _native.ABI_VERSION == 15 and native_lib.sfm_abi_version() == 15   # the change is additive
    with open(os.path.join(REPO, "include", "sfm_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint sfm_pair_poses\s*\(", header) and "typedef struct sfm_pair_pose" in header
    assert re.search(r"\bint64_t sfm_pair_poses_workspace_bytes\s*\(", header)
    for code, name in enumerate(("OK", "NO_MODEL", "NOT_ESSENTIAL", "NO_VOTE", "BAD_OFFSETS")):
        assert re.search(rf"#define SFM_POSE_{name} {code}\b", header)
    assert "sfm_pair_poses" in _native.SIGNATURES and native_lib.sfm_pair_poses is not None
    assert "sfm_pair_poses_workspace_bytes" in _native.OTHER_SYMBOLS
    assert C.sizeof(_native.PairPose) == 128 and device.POSE_BYTES == 128 and device.POSE_DTYPE.itemsize == 128
    assert [(n, device.POSE_DTYPE.fields[n][1]) for n in device.POSE_DTYPE.names] == [
        (n, getattr(_native.PairPose, n).offset) for n, _ in _native.PairPose._fields_]
    assert device.POSE_STATUS == ("ok", "no_model", "not_essential", "no_vote", "bad_offsets") == po.STATUS
    assert (device.POSE_OK, device.POSE_NO_MODEL, device.POSE_NOT_ESSENTIAL, device.POSE_NO_VOTE, device.POSE_BAD_OFFSETS) == (
        po.OK, po.NO_MODEL, po.NOT_ESSENTIAL, po.NO_VOTE, po.BAD_OFFSETS)
    assert hasattr(device.ViewGraphWorkspace, "poses")
    op = ops.load()
    assert "pair_poses" in ops.FUNCTIONAL_OPS
    schema = str(op.pair_poses.default._schema)
    assert schema.startswith("sfm_hip::pair_poses(Tensor corr, Tensor offset, Tensor E, Tensor e_result, Tensor e_mask, Tensor verdict, "
                             "float distance_threshold)") and schema.endswith("-> (Tensor, Tensor)")
    import lib.epipolar.view_graph as drop_in

    assert drop_in.PairPoses is vg.PairPoses and drop_in.verify_pairs is vg.verify_pairs
    assert vg.ViewGraph._fields[-1] == "pose" and vg.ViewGraph._field_defaults == {"pose": None}
    assert vg.PairPoses._fields == ("R", "t", "votes", "in_front", "median_angle_deg", "status")


def test_meta_kernel_shapes():
    import torch

    from structure_from_motion_amd import ops

    op = ops.load()
    meta = lambda shape, dtype: torch.empty(shape, dtype=dtype, device="meta")   # noqa: E731
    pose, angle = op.pair_poses(meta((100, 4), torch.float64), meta((4,), torch.int64), meta((3, 7, 9), torch.float64),
                                meta((3, 5), torch.int64), meta((100,), torch.uint8), meta((3, 3), torch.int64), 50.0)
    assert pose.shape == (3, 128) and pose.dtype == torch.uint8 and angle.shape == (100,) and angle.dtype == torch.float64


def _call(lib, n_total=100, pairs=3, h=10, workspace_bytes=None, null=()):
    """``sfm_pair_poses`` with host addresses that a refused call never follows."""
    scratch = (C.c_double * 16)()
    p = {name: (None if name in null else C.addressof(scratch))
         for name in ("corr", "offset", "E", "e_result", "e_mask", "verdict", "pose", "workspace")}
    if workspace_bytes is None:
        workspace_bytes = 0
    return lib.sfm_pair_poses(p["corr"], n_total, p["offset"], pairs, p["E"], h, p["e_result"], p["e_mask"], p["verdict"], 50.0,
                              p["pose"], p["workspace"], workspace_bytes, None)


def test_entry_refuses_bad_arguments_before_any_launch(native_lib):
    lib = native_lib
    for kwargs in (dict(n_total=-1), dict(pairs=-1), dict(pairs=65536), dict(n_total=2**31), dict(h=0), dict(h=-1), dict(h=2**31)):
        assert _call(lib, **kwargs) == EINVAL, kwargs
    assert _call(lib, pairs=65536) == EINVAL and b"65535" in lib.sfm_last_error()
    assert _call(lib, n_total=2**31) == EINVAL and b"2^31" in lib.sfm_last_error()
    assert _call(lib, h=0) == EINVAL and b"h_count" in lib.sfm_last_error()
    for name in ("corr", "offset", "E", "e_result", "e_mask", "verdict", "pose", "workspace"):
        assert _call(lib, null=(name,), workspace_bytes=2**40) == EINVAL and b"null pointer" in lib.sfm_last_error(), name
    need = lib.sfm_pair_poses_workspace_bytes(100, 3)
    assert need >= 8 * 100   # the angle of every item comes first
    assert _call(lib, workspace_bytes=need - 1) == EINVAL and b"workspace" in lib.sfm_last_error()
    assert _call(lib, workspace_bytes=0) == EINVAL
    assert _call(lib, pairs=0) == 0   # no pairs: a no-op
    assert lib.sfm_pair_poses_workspace_bytes(0, 0) == 0
    assert lib.sfm_pair_poses_workspace_bytes(101, 3) > need and lib.sfm_pair_poses_workspace_bytes(100, 4) > need
    for bad in ((-1, 3), (100, -1), (2**31, 3), (100, 65536)):
        assert lib.sfm_pair_poses_workspace_bytes(*bad) == -1, bad


def _graph(sizes=(10, 12)):
    rng = np.random.default_rng(3)
    features, pairs, matches = [], [], []
    for q, n in enumerate(sizes):
        features += [rng.uniform(0, 600, (n, 2)), rng.uniform(0, 600, (n, 2))]
        pairs.append((2 * q, 2 * q + 1))
        matches.append(np.column_stack([np.arange(n), np.arange(n)]))
    return features, pairs, matches


def test_verify_pairs_refuses_bad_pose_arguments_before_device_work():
    features, pairs, matches = _graph()
    for distance in (0.0, -1.0, float("nan"), float("inf")):
        for relative_pose in (False, True):
            with pytest.raises(ValueError, match="distance_threshold"):
                vg.verify_pairs(K, features, pairs, matches, 2e-5, relative_pose=relative_pose, distance_threshold=distance)
    with pytest.raises(ValueError, match="max_iterations"):
        vg.verify_pairs(K, features, pairs, matches, 2e-5, relative_pose=True, max_iterations=0)
    # the earlier checks still come first, and no pairs is an empty graph with an empty pose table, no device
    with pytest.raises(ValueError, match="one entry per pair"):
        vg.verify_pairs(K, features, pairs, matches[:1], 2e-5, relative_pose=True)
    empty = vg.verify_pairs(K, features, [], [], 2e-5, relative_pose=True)
    assert empty.pose.R.shape == (0, 3, 3) and empty.pose.t.shape == (0, 3) and empty.pose.votes.shape == (0, 4)
    assert empty.pose.status == [] and len(empty.pose.in_front) == 0 and len(empty.pose.median_angle_deg) == 0
    assert vg.verify_pairs(K, features, [], [], 2e-5).pose is None


# The candidates have a unit baseline, so points come out in units of it: bench_narrow's lie at 5 / 0.0256 = 195 of them, beyond
# the default distance threshold of 50 (which therefore also bounds the parallax from below, at about 1 / 50 rad = 1.1 degrees).
@pytest.mark.parametrize("name, distance", [("bench", 50.0), ("gen12_t", 50.0), ("bench_narrow", 1000.0)])
def test_oracle_recovers_the_true_pose_and_parallax(name, distance):
    n, seed = 300, 13
    sc = po.motion_scene(name, n, seed)
    X = po.scene_points(name, n, seed)
    Kc = sc["K"]
    uvw = X @ Kc.T
    assert np.allclose(uvw[:, :2] / uvw[:, 2:3], sc["pix_a"], rtol=0, atol=1e-9)   # these are the scene's points
    R, t = sc["R"], sc["t"]
    got = po.pair_pose(sc["corr"], np.ones(n, np.uint8), po.essential(R, t), distance)
    if name == "bench_narrow":
        assert po.pair_pose(sc["corr"], np.ones(n, np.uint8), po.essential(R, t), 50.0)["status"] == po.NO_VOTE
    assert got["status"] == po.OK and got["votes"][got["best"]] == n and sorted(got["votes"])[:3] == [0, 0, 0]
    np.testing.assert_allclose(got["R"], R, rtol=0, atol=1e-12)
    np.testing.assert_allclose(got["t"], t / np.linalg.norm(t), rtol=0, atol=1e-12)
    truth = po.true_parallax(X, R, t)
    np.testing.assert_allclose(got["angles"], truth, rtol=0, atol=1e-9)
    assert abs(got["median_angle"] - np.sort(truth)[(n - 1) // 2]) <= 1e-9
    # a mask is honoured: the items it leaves out neither vote nor have an angle
    mask = (np.arange(n) % 3 != 0).astype(np.uint8) * 2
    part = po.pair_pose(sc["corr"], mask, po.essential(R, t), distance)
    assert part["votes"][part["best"]] == np.count_nonzero(mask) and np.array_equal(np.isnan(part["angles"]), mask == 0)
    assert part["median_angle"] == po.lower_median(got["angles"][mask != 0])


def test_motion_parallax_figures():
    """bench_narrow's parallax is a twentieth of bench's: about 0.29 against 5.7 degrees."""
    medians = {}
    for name in ("bench", "bench_narrow"):
        R, t, _ = po.MOTIONS[name]
        medians[name] = np.degrees(np.median(po.true_parallax(po.scene_points(name, 400, 7), R, t)))
    assert 5.0 < medians["bench"] < 6.5 and 0.25 < medians["bench_narrow"] < 0.33
    assert np.array_equal(po.MOTIONS["bench_narrow"][0], po.MOTIONS["bench"][0])


KIND_DISTANCE = 1000.0   # the distance at which the GPU test compares the medians of the kind scenes (bench_narrow has voters)


def test_kind_scene_medians_are_ordered_under_the_cpu_oracle():
    """The condition the GPU test of the kinds asserts, first on the CPU: with a RANSAC of the oracle on each kind scene (its
    eight-point fit on Philox samples, 200 hypotheses, the GPU test's gate) and the NumPy pose definition on that winner's
    inliers, bench's median angle is above 2 degrees and above that of both pure rotations, pan10 and gen12, whose matrices
    are fits to noise.  The votes of these matrices rest on no near-tie either."""
    from oracle import sfm_oracle as orc

    median = {}
    for q, ((name, n), sc) in enumerate(zip(po.KIND_CASES, po.kind_scenes())):
        S = orc.philox_sample_table(5 + q, 0, 200, n)
        r = orc.ransac_essential(sc["corr"], S, vo.THR, min_extra=max(8, n // 15))
        assert r["best"] >= 0, name
        mask = np.zeros(n, np.uint8)
        mask[r["inliers"]] = 1
        for pose in po.candidates(r["E"])[::2]:
            depth, norm = po.cheirality_margins(sc["corr"][mask != 0], pose[:9].reshape(3, 3), pose[9:], KIND_DISTANCE)
            assert depth > 1e-6 and norm > 1e-6, (name, depth, norm)
        got = po.pair_pose(sc["corr"], mask, r["E"], KIND_DISTANCE)
        assert got["status"] in (po.OK, po.NO_VOTE), name
        median[name] = np.degrees(got["median_angle"])   # NaN when nobody votes
    print("median angle in degrees by kind scene:", median)
    assert median["bench"] > 2.0
    for name in ("pan10", "gen12"):
        assert not median[name] >= median["bench"], (name, median)
        if not np.isnan(median[name]):
            print(name, "bench / this median:", median["bench"] / median[name])


def test_oracle_statuses():
    sc = po.motion_scene("bench", 50, 3)
    ones = np.ones(50, np.uint8)
    assert po.pair_pose(sc["corr"], ones, None)["status"] == po.NO_MODEL
    assert po.pair_pose(sc["corr"], ones, np.eye(3))["status"] == po.NOT_ESSENTIAL
    E = po.essential(sc["R"], sc["t"])
    none = po.pair_pose(sc["corr"], np.zeros(50, np.uint8), E)   # nobody votes
    assert none["status"] == po.NO_VOTE and none["best"] == -1 and not none["votes"].any() and np.isnan(none["R"]).all()
    far = po.pair_pose(sc["corr"], ones, E, distance_threshold=1.0)   # every point is farther than that
    assert far["status"] == po.NO_VOTE and np.isnan(far["angles"]).all()
    assert po.lower_median(np.array([3.0, 1.0])) == 1.0 and po.lower_median(np.array([3.0, 1.0, 2.0])) == 2.0
    assert po.lower_median(np.array([4.0, 3.0, 1.0, 2.0])) == 2.0


def _table(kinds, e_counts, ratios, angles=None, status=None):
    Q = len(kinds)
    none = np.full((Q, 3, 3), np.nan)
    pose = None
    if angles is not None:
        pose = vg.PairPoses(none, np.full((Q, 3), np.nan), np.zeros((Q, 4), np.int64), np.zeros(Q, np.int64),
                            np.array(angles, dtype=np.float64), list(status or ["ok"] * Q))
    return vg.ViewGraph(np.zeros((Q, 2), dtype=np.int64), list(kinds), none, none, np.array(e_counts, dtype=np.int64),
                        np.zeros(Q, dtype=np.int64), np.array(ratios, dtype=np.float64), [None] * Q, [None] * Q, [None] * Q, pose)


def test_choose_seed_pair_angle_gate():
    kinds = ["homography", "essential", "essential", "essential", "essential"]
    counts, ratios = [283, 260, 187, 150, 75], [0.99, 0.3, 0.15, 0.2, 0.1]
    angles = [0.01, 0.29, 5.7, np.nan, 9.0]
    status = ["ok", "ok", "ok", "no_vote", "ok"]
    g = _table(kinds, counts, ratios, angles, status)
    # defaults: today's answer, with or without a pose table
    assert vg.choose_seed_pair(g) == 1 == vg.choose_seed_pair(_table(kinds, counts, ratios))
    assert vg.choose_seed_pair(g, min_count=188) == 1 and vg.choose_seed_pair(g, 0, 0.0) == 1
    # the gate: the narrow pair goes, the ranking of the rest is unchanged
    assert vg.choose_seed_pair(g, min_angle_deg=0.29) == 1
    assert vg.choose_seed_pair(g, min_angle_deg=0.3) == 2
    assert vg.choose_seed_pair(g, min_angle_deg=2.0) == 2
    assert vg.choose_seed_pair(g, min_angle_deg=5.8) == 4
    assert vg.choose_seed_pair(g, min_count=76, min_angle_deg=2.0) == 2
    with pytest.raises(ValueError, match="no pair"):
        vg.choose_seed_pair(g, min_count=76, min_angle_deg=5.8)
    with pytest.raises(ValueError, match="no pair"):
        vg.choose_seed_pair(g, min_angle_deg=9.5)
    # a status other than "ok" is never eligible under a gate, whatever its angle says
    odd = _table(["essential", "essential"], [100, 50], [0.1, 0.1], [8.0, 3.0], ["not_essential", "ok"])
    assert vg.choose_seed_pair(odd) == 0 and vg.choose_seed_pair(odd, min_angle_deg=1.0) == 1
    # ties still go to the lower ratio, then to the lower index
    tie = _table(["essential"] * 3, [120, 120, 120], [0.3, 0.2, 0.2], [4.0, 4.0, 4.0])
    assert vg.choose_seed_pair(tie, min_angle_deg=2.0) == 1
    # a gate without a pose table
    with pytest.raises(ValueError, match="relative_pose"):
        vg.choose_seed_pair(_table(kinds, counts, ratios), min_angle_deg=2.0)
    # ten positional values still build a graph
    assert vg.ViewGraph(*([None] * 10)).pose is None


def _fixture_pairs():
    """(label, corr, R, t) of every pair of the GPU fixtures whose scene has a baseline."""
    out = []
    for k, sc in enumerate(vo.ragged_scenes()):
        out.append((f"ragged {k}", sc["corr"], sc["R"], sc["t"], po.DISTANCE))
    for (name, n), sc in zip(po.KIND_CASES, po.kind_scenes()):
        for distance in (po.DISTANCE, KIND_DISTANCE):   # the GPU test runs these scenes at both
            out.append((f"kinds {name} at {distance}", sc["corr"], sc["R"], sc["t"], distance))
    corr, offset, _, R, t = po.edge_case_fixture()
    for q in range(len(offset) - 1):
        out.append((f"edge {q}", corr[offset[q]:offset[q + 1]], R, t, po.DISTANCE))
    return out


def test_fixture_votes_rest_on_no_near_tie():
    """Under the true pose of every fixture pair that has one, and its mirror, and under the twisted pair of that essential
    matrix, no item's depths lie within 1e-6 of -1e-8 (or of +1e-8, the same test under the mirrored pose) and no norm within
    1e-6 relative of the threshold.  A pure rotation has no true essential matrix: those pairs are covered by the matrices an
    oracle RANSAC selects (here for the ragged scenes, in the ordering test above for the kind scenes).  The device's five-point
    winners are other matrices again: the GPU tests assert the same margins on the device's own poses before comparing votes."""
    checked = 0
    for label, corr, R, t, distance in _fixture_pairs():
        if not np.any(t) or len(corr) == 0:
            continue
        for pose in po.candidates(po.essential(R, t))[::2]:
            depth, norm = po.cheirality_margins(corr, pose[:9].reshape(3, 3), pose[9:], distance)
            assert depth > 1e-6 and norm > 1e-6, (label, depth, norm)
            checked += 1
    assert checked == 2 * (5 + 2 * 3 + 10)
    # and under the best and the mirrored poses of the matrix a RANSAC of the oracle selects on each ragged scene (its
    # eight-point fit: pure rotations and planes included, whose winners are fits to noise like the device's)
    from oracle import sfm_oracle as orc

    selected = 0
    for k, sc in enumerate(vo.ragged_scenes()):
        n = len(sc["corr"])
        if n < 8:
            continue
        r = orc.ransac_essential(sc["corr"], orc.philox_sample_table(40 + k, 0, 256, n), vo.THR, min_extra=n // 15)
        if r["best"] < 0:
            continue
        for pose in po.candidates(r["E"])[::2]:
            depth, norm = po.cheirality_margins(sc["corr"][r["inliers"]], pose[:9].reshape(3, 3), pose[9:])
            assert depth > 1e-6 and norm > 1e-6, (k, depth, norm)
        selected += 1
    assert selected >= 4
