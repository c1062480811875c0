"""Relative pose and triangulation angle per pair behind the view-graph call on the GPU (csrc/sfm_view_graph_pose.hip, DESIGN.md
§6r): the ragged fixture against the NumPy definition, the exact selection of the median on hand-built pairs, the kinds and the
seed pair, chunking and determinism, refused offset tables, the op and the app."""
import numpy as np
import pytest
import torch

import view_graph_oracle as vo
import view_graph_pose_oracle as po
from structure_from_motion_amd import synthetic

pytestmark = pytest.mark.gpu

K = synthetic.BENCH_K
THR = vo.THR
SEED = 0x9E3779B97F4A7C15
MAX_RATIO = 0.8
H = 256
MEDIAN_ATOL = 1e-13   # ~300 x the rounding of a cross product at |a||c| <= 3 plus a 2-ulp atan2
SET_ATOL = 1e-10      # the decomposition parity test's (tests/test_gpu_parity.py::test_decompose_essential)
MARGIN = 1e-6         # no cheirality test of a compared vote is this close to its limit


@pytest.fixture(scope="module")
def dev(native_lib):
    from structure_from_motion_amd import device

    return device.require_gpu()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _pose_set_equal(got, want, atol):
    """The four candidates of one decomposition equal those of the other as a set."""
    return all(any(np.allclose(g, w, rtol=0, atol=atol) for g in got) for w in want)


@pytest.fixture(scope="module")
def ragged(dev):
    """The 12-pair fixture after one verify call and one pose call (computed once, never written)."""
    from structure_from_motion_amd import device

    scenes = vo.ragged_scenes()
    corr, offset, min_extra = vo.ragged_arrays(scenes)
    Q, N = len(vo.SIZES), len(corr)
    ws = device.ViewGraphWorkspace(Q, N, H, dev)
    corr_t, offset_t = device.to_device(corr), device.to_device(offset, torch.int64)
    ws.run(corr_t, offset_t, device.to_device(min_extra), THR, vo.RMS, MAX_RATIO, SEED)
    ws.poses(po.DISTANCE)
    best_h = ws.e_result[:, 1].cpu().numpy()
    rows = torch.arange(Q, device=dev)
    E = ws.E[rows, ws.e_result[:, 1].clamp(min=0)]   # [Q, 9], the winners (row 0 where there is none)
    cand, cand_status = device.decompose_essential(E.contiguous())
    return dict(scenes=scenes, corr=corr, offset=offset, ws=ws, corr_t=corr_t, offset_t=offset_t, best_h=best_h,
                E=E.cpu().numpy(), cand=cand.cpu().numpy(), cand_status=cand_status.cpu().numpy(),
                e_mask=ws.e_mask.cpu().numpy(), pose=po.decode(ws.pose.cpu().numpy()), angle=ws.angle.cpu().numpy(),
                outcome=ws.outcome())


def _assert_filler(p, status):
    assert p["status"] == status and np.isnan(p["R"]).all() and np.isnan(p["t"]).all() and np.isnan(p["median_angle"])
    assert not p["votes"].any() and p["best"] == -1


def test_ragged_parity(ragged):
    corr, offset, pose, angle = ragged["corr"], ragged["offset"], ragged["pose"], ragged["angle"]
    assert len(angle) == len(corr) and len(pose) == len(vo.SIZES)
    n_ok = 0
    for q, n in enumerate(vo.SIZES):
        lo, hi = offset[q], offset[q + 1]
        c, mask, got = corr[lo:hi], ragged["e_mask"][lo:hi], pose[q]
        if ragged["best_h"][q] < 0:   # no_model exactly where E has no winner
            _assert_filler(got, po.NO_MODEL)
            assert np.isnan(angle[lo:hi]).all()
            continue
        assert got["status"] != po.NO_MODEL and ragged["cand_status"][q] == 0 and got["status"] in (po.OK, po.NO_VOTE), q
        cand = ragged["cand"][q]
        # the candidates against the NumPy decomposition of the device's E
        assert _pose_set_equal(cand, po.candidates(ragged["E"][q]), SET_ATOL), q
        # the exact comparison below rests on no near-tie: the device's own poses, both rotations, mirrors included
        items = c[mask != 0]
        for k in (0, 2):
            depth, norm = po.cheirality_margins(items, cand[k][:9].reshape(3, 3), cand[k][9:])
            print(f"pair {q} n {n} candidate {k}: depth margin {depth:.3e} norm margin {norm:.3e}")
            assert depth > MARGIN and norm > MARGIN, (q, k, depth, norm)
        want = po.pair_pose(c, mask, ragged["E"][q], po.DISTANCE, poses=cand)
        print(f"pair {q} n {n}: votes {got['votes']} oracle {want['votes']} best {got['best']} median {got['median_angle']!r} "
              f"oracle {want['median_angle']!r}")
        assert np.array_equal(got["votes"], want["votes"]) and got["best"] == want["best"], q
        assert got["status"] == want["status"], q
        if want["status"] != po.OK:
            _assert_filler(got, po.NO_VOTE)
            assert np.isnan(angle[lo:hi]).all()
            continue
        n_ok += 1
        # the pose is the winning candidate of sfm_decompose_essential, bit for bit
        assert np.array_equal(_bits(got["R"]), _bits(cand[got["best"]][:9].reshape(3, 3))), q
        assert np.array_equal(_bits(got["t"]), _bits(cand[got["best"]][9:])), q
        assert abs(got["median_angle"] - want["median_angle"]) <= MEDIAN_ATOL, q
        # the angle buffer: NaN exactly off the passing inliers, the oracle's angles on them
        seg = angle[lo:hi]
        assert np.array_equal(np.isnan(seg), np.isnan(want["angles"])), q
        on = ~np.isnan(seg)
        k = int(got["votes"][got["best"]])
        assert np.count_nonzero(on) == k and np.all(np.abs(seg[on] - want["angles"][on]) <= MEDIAN_ATOL), q
        # the median is selected exactly from the device's own angles
        assert _bits(got["median_angle"]) == _bits(np.sort(seg)[(k - 1) // 2]), q
    assert n_ok >= 4   # the fixture is not vacuous: the large pairs with a baseline have a pose
    # the decoded fields of the workspace are the table
    out = ragged["outcome"]
    assert np.array_equal(out.pose_status, [p["status"] for p in pose]) and np.array_equal(out.pose_best, [p["best"] for p in pose])
    assert np.array_equal(_bits(out.pose_R), _bits(np.array([p["R"] for p in pose])))
    assert np.array_equal(_bits(out.pose_median_angle), _bits(np.array([p["median_angle"] for p in pose])))
    assert np.array_equal(out.pose_votes, np.array([p["votes"] for p in pose]))


def _hand_built(dev, corr, offset, e_mask, E_rows, best_h, kind=vo.ESSENTIAL):
    """The tensors of a ``pair_poses`` call with one hypothesis per pair: E_rows (Q, 9), best_h (Q,)."""
    from structure_from_motion_amd import device

    Q = len(offset) - 1
    result = np.zeros((Q, 5), dtype=np.int64)
    result[:, 1] = best_h
    verdict = np.zeros((Q, 3), dtype=np.int64)
    verdict[:, 0] = kind   # the low word of the first int64 is the kind
    return (device.to_device(corr), device.to_device(offset, torch.int64), device.to_device(np.asarray(E_rows).reshape(Q, 1, 9)),
            device.to_device(result, torch.int64), device.to_device(e_mask, torch.uint8), device.to_device(verdict, torch.int64))


def test_selection_edge_cases(dev):
    from structure_from_motion_amd import ops

    corr, offset, e_mask, R, t = po.edge_case_fixture()
    Q = len(offset) - 1
    E = po.essential(R, t)
    args = _hand_built(dev, corr, offset, e_mask, np.tile(E.reshape(1, 9), (Q, 1)), np.zeros(Q, np.int64))
    pose_t, angle_t = ops.load().pair_poses(*args, po.DISTANCE)
    pose, angle = po.decode(pose_t.cpu().numpy()), angle_t.cpu().numpy()
    expected_k = list(po.EDGE_COUNTS) + [257, 600, 601, 300]
    for q in range(Q):
        lo, hi = offset[q], offset[q + 1]
        got, seg, k = pose[q], angle[lo:hi], expected_k[q]
        assert got["status"] == po.OK and got["votes"][got["best"]] == k, (q, got)
        np.testing.assert_allclose(got["R"], R, rtol=0, atol=1e-12)
        np.testing.assert_allclose(got["t"], t / np.linalg.norm(t), rtol=0, atol=1e-12)
        assert np.array_equal(np.isnan(seg), e_mask[lo:hi] == 0), q
        want = po.ray_angles(corr[lo:hi], got["R"])
        on = e_mask[lo:hi] != 0
        assert np.all(np.abs(seg[on] - want[on]) <= MEDIAN_ATOL), q
        ordered = np.sort(seg)
        print(f"pair {q}: k {k} median {got['median_angle']!r} neighbours {ordered[max((k - 1) // 2 - 1, 0):(k - 1) // 2 + 2]!r}")
        assert _bits(got["median_angle"]) == _bits(ordered[(k - 1) // 2]), q
    # the fixture has the cases it names: one key, two keys with the rank on their boundary, keys apart in the last digit only
    assert len(np.unique(_bits(angle[offset[7]:offset[8]]))) == 1
    two = np.sort(angle[offset[8]:offset[9]])
    assert len(np.unique(_bits(two))) == 2 and (two[299] != two[300] or two[300] != two[301])
    ulps = _bits(angle[offset[9]:offset[10]])
    assert len(np.unique(ulps)) > 8 and np.ptp(ulps) < 4096


def test_kinds_and_seed_pair(dev):
    from lib.epipolar.eight_point import recover_r_t_from_e
    from lib.common.feature import Feature
    from apps.sfm_multi_view import rotation_angle
    from structure_from_motion_amd.epipolar import view_graph as vg

    scenes = po.kind_scenes()
    names = [name for name, _ in po.KIND_CASES]
    features, pairs, matches = vo.match_graph(scenes)
    gate = [max(8, n // 15) for _, n in po.KIND_CASES]
    # 1 000 baselines: bench_narrow's points lie 195 of its baselines away, beyond the default 50 (looked at further down)
    graph = vg.verify_pairs(K, features, pairs, matches, THR, min_num_extra_inliers=gate, max_iterations=200, seed=5,
                            relative_pose=True, distance_threshold=1000.0)
    pose = graph.pose
    print("kinds", graph.kind, "E", graph.essential_count, "ratio", graph.ratio, "status", pose.status, "median deg",
          pose.median_angle_deg, "in front", pose.in_front, "votes", pose.votes.tolist())
    assert all(np.isfinite(graph.E[q]).all() for q in range(5))   # every pair has an E winner here
    assert all(s in ("ok", "no_vote") for s in pose.status)
    narrow, bench = names.index("bench_narrow"), names.index("bench")
    assert pose.status[bench] == "ok" and pose.status[narrow] == "ok"
    assert pose.median_angle_deg[bench] > 2.0 > pose.median_angle_deg[narrow]
    for q, name in enumerate(names):   # a rotation's pair has no parallax to speak of (NaN when nobody votes)
        if name in ("pan10", "gen12"):
            assert not pose.median_angle_deg[q] >= pose.median_angle_deg[bench], (name, pose.median_angle_deg[q])
            if pose.status[q] == "ok":
                print(name, "bench / this median:", pose.median_angle_deg[bench] / pose.median_angle_deg[q])
    assert vg.choose_seed_pair(graph, min_angle_deg=2.0) == bench
    for q in range(5):
        assert pose.in_front[q] == (pose.votes[q].max() if pose.status[q] == "ok" else 0)
        assert pose.in_front[q] <= graph.essential_count[q]
    # bench's R is as good as the one the same E gives through recover_r_t_from_e on the same inliers
    m = graph.essential_inliers[bench]
    fa = [Feature(float(x), float(y)) for x, y in features[2 * bench][m[:, 0]]]
    fb = [Feature(float(x), float(y)) for x, y in features[2 * bench + 1][m[:, 1]]]
    R_ref, t_ref, _ = recover_r_t_from_e(graph.E[bench], K, fa, fb, 1000.0)
    truth = scenes[bench]["R"]
    err, err_ref = rotation_angle(pose.R[bench], truth), rotation_angle(np.asarray(R_ref), truth)
    print("bench rotation error", err, "through recover_r_t_from_e", err_ref)
    assert err <= err_ref + 1e-9   # the same matrix decomposed by the same routine: rounding of the arc cosine at most
    assert np.dot(pose.t[bench], scenes[bench]["t"]) > 0.0
    # the default distance, which the app and every caller who passes none gets.  The distance enters the norm test alone, so
    # no vote can grow from 1 000 to 50.  bench_narrow's points lie 156 .. 234 of its baselines away (depths 4 .. 6 over a
    # baseline of 0.0256): none of them is within 50, and only an outlier that happens to lie on its epipolar line, at whatever
    # depth that gives it, can vote.  The pair is no_vote or rests on those few (2 of 283 inliers in the recorded run, median
    # 1.48 degrees), and the gate still finds bench.
    default = vg.verify_pairs(K, features, pairs, matches, THR, min_num_extra_inliers=gate, max_iterations=200, seed=5,
                              relative_pose=True)
    dpose = default.pose
    print("default distance: status", dpose.status, "median deg", dpose.median_angle_deg, "votes", dpose.votes.tolist())
    _same_graph(default, graph)   # the distance is no input of the verify call
    assert np.all(dpose.votes <= pose.votes)
    chance = int(np.count_nonzero(scenes[narrow]["is_outlier"][default.essential_inliers[narrow][:, 0]]))
    print("bench_narrow at the default: in front", dpose.in_front[narrow], "outliers among its inliers", chance)
    assert dpose.status[narrow] in ("ok", "no_vote") and dpose.in_front[narrow] <= chance
    assert dpose.status[bench] == "ok" and dpose.median_angle_deg[bench] > 2.0
    assert vg.choose_seed_pair(default, min_angle_deg=2.0) == bench


def _same_graph(a, b):
    assert a.kind == b.kind and np.array_equal(a.pairs, b.pairs)
    for name in ("E", "H", "ratio"):
        assert np.array_equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name
    assert np.array_equal(a.essential_count, b.essential_count) and np.array_equal(a.homography_count, b.homography_count)
    for name in ("essential_inliers", "homography_inliers", "inlier_matches"):
        assert all(np.array_equal(x, y) for x, y in zip(getattr(a, name), getattr(b, name))), name


def _same_pose(a, b):
    for name in ("R", "t", "median_angle_deg"):
        assert np.array_equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name
    assert np.array_equal(a.votes, b.votes) and np.array_equal(a.in_front, b.in_front) and a.status == b.status


def test_chunking_and_determinism(dev, ragged):
    from structure_from_motion_amd.epipolar import view_graph as vg

    features, pairs, matches = vo.match_graph(ragged["scenes"])
    h = 64
    assert len(vg.chunk_bounds(len(pairs), h, 4 * h)) == 3
    args = (K, features, pairs, matches, THR)
    kwargs = dict(min_extra_fraction=1.0 / 15.0, max_iterations=h, seed=11)
    whole = vg.verify_pairs(*args, **kwargs, relative_pose=True)
    again = vg.verify_pairs(*args, **kwargs, relative_pose=True)
    chunked = vg.verify_pairs(*args, **kwargs, relative_pose=True, max_hypotheses_per_call=4 * h)
    plain = vg.verify_pairs(*args, **kwargs)
    assert plain.pose is None and whole.pose is not None
    for other in (again, chunked):
        _same_graph(whole, other)
        _same_pose(whole.pose, other.pose)
    _same_graph(whole, plain)   # every field there was is what it was
    small = sum(n < vo.E_SAMPLE for n in vo.SIZES)   # the pairs too small for an essential matrix come first: 0, 3, 4, 5 items
    assert small == 4 and whole.pose.status[:small] == ["no_model"] * small and "ok" in whole.pose.status
    assert all((s == "ok") == bool(np.isfinite(whole.pose.R[q]).all()) for q, s in enumerate(whole.pose.status))


def test_bad_offsets_are_a_status(dev, ragged):
    from structure_from_motion_amd import device, ops

    offset = ragged["offset"].copy()
    offset[8], offset[9] = offset[9], offset[8]   # decreasing
    Q, N = len(vo.SIZES), len(ragged["corr"])
    ws = device.ViewGraphWorkspace(Q, N, 65, dev)
    ws.run(ragged["corr_t"], device.to_device(offset, torch.int64), device.to_device(np.full(Q, 5.0)), THR, vo.RMS,
           MAX_RATIO, SEED)
    ws.poses(po.DISTANCE)   # returns: a status, not a fault
    assert all(v.kind == vo.BAD_OFFSETS for v in ws.read_verdicts())
    for p in po.decode(ws.pose.cpu().numpy()):
        _assert_filler(p, po.BAD_OFFSETS)
    assert np.isnan(ws.angle.cpu().numpy()).all()
    assert np.all(ws.outcome().pose_status == device.POSE_BAD_OFFSETS)
    # the mark alone decides: a table that would index far outside, with records that name a winner, is never followed
    corr, _, e_mask, R, t = po.edge_case_fixture()
    wild = np.array([0, 2**40, -2**40, len(corr)], dtype=np.int64)
    E = np.tile(po.essential(R, t).reshape(1, 9), (3, 1))
    args = _hand_built(dev, corr, wild, e_mask, E, np.zeros(3, np.int64), kind=vo.BAD_OFFSETS)
    pose_t, angle_t = ops.load().pair_poses(*args, po.DISTANCE)
    for p in po.decode(pose_t.cpu().numpy()):
        _assert_filler(p, po.BAD_OFFSETS)
    assert np.isnan(angle_t.cpu().numpy()).all()


BYTE_SENTINEL, F64_SENTINEL = 77, 1e300
WORD64_SENTINEL = int.from_bytes(bytes([BYTE_SENTINEL] * 8), "little")   # a pose field nobody wrote, as its 8 or 4 bytes
WORD32_SENTINEL = int.from_bytes(bytes([BYTE_SENTINEL] * 4), "little")


def _prefilled_call(lib, corr, offset, E, e_result, e_mask, verdict, distance):
    """``sfm_pair_poses`` itself on a pose table of sentinel bytes and a workspace of sentinel doubles: every field of every
    record and every item's angle must have been written over -> (pose uint8 (Q, 128), angle (N,)) on the host."""
    N, Q = corr.shape[0], offset.numel() - 1
    need = lib.sfm_pair_poses_workspace_bytes(N, Q)
    assert need >= 8 * N
    pose = torch.full((Q, po.POSE_BYTES), BYTE_SENTINEL, dtype=torch.uint8, device=corr.device)
    workspace = torch.full(((need + 7) // 8,), F64_SENTINEL, dtype=torch.float64, device=corr.device)
    for t in (corr, offset, E, e_result, e_mask, verdict):
        assert t.is_contiguous()
    rc = lib.sfm_pair_poses(corr.data_ptr(), N, offset.data_ptr(), Q, E.data_ptr(), E.shape[1], e_result.data_ptr(),
                            e_mask.data_ptr(), verdict.data_ptr(), float(distance), pose.data_ptr(), workspace.data_ptr(), need,
                            torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.sfm_last_error()
    pose_h, angle_h = pose.cpu().numpy(), workspace[:N].cpu().numpy()
    doubles = pose_h[:, :104].copy().view(np.int64)   # R, t, median_angle
    ints = pose_h[:, 104:].copy().view(np.int32)      # votes, best, status
    assert doubles.shape == (Q, 13) and ints.shape == (Q, 6)
    assert not np.any(doubles == WORD64_SENTINEL) and not np.any(ints == WORD32_SENTINEL)
    assert not np.any(angle_h == F64_SENTINEL)
    return pose_h, angle_h


def _assert_same_bits(pose_h, angle_h, pose_t, angle_t):
    assert np.array_equal(pose_h, pose_t.cpu().numpy()) and np.array_equal(_bits(angle_h), _bits(angle_t.cpu().numpy()))


def _four_statuses(dev):
    """no_model, not_essential, no_vote and ok side by side in one hand-built call, with items no pair owns."""
    sc = po.motion_scene("bench", 40, 5)
    n = 40
    corr = np.concatenate([sc["corr"]] * 5)           # five runs of the same 40 items: the first and the last belong to no pair
    offset = np.array([n, 2 * n, 3 * n, 4 * n, 4 * n], dtype=np.int64)   # four pairs, the last one empty
    e_mask = np.ones(5 * n, dtype=np.uint8)
    e_mask[2 * n:3 * n] = 0                             # pair 1: nobody votes
    E = np.stack([po.essential(sc["R"], sc["t"]).reshape(9)] * 4)
    E[2] = np.eye(3).reshape(9)                          # pair 2: full rank
    best_h = np.array([0, 0, 0, -1], dtype=np.int64)    # pair 3: no winner
    return sc, n, corr, offset, e_mask, E, best_h


def test_every_output_byte_is_written(dev, ragged, native_lib):
    """The entry on prefilled buffers: no sentinel survives in pose [Q, 128] or in the angle of an item, on the path of every
    status (the filler of launch 1, the status-only write of launch 1 completed by launch 3), for items no pair owns and under
    a refused offset table; and the result is the op's, bit for bit."""
    from structure_from_motion_amd import device, ops

    op = ops.load()
    # the four statuses side by side, items before the first pair and after the last
    _, n, corr, offset, e_mask, E, best_h = _four_statuses(dev)
    args = _hand_built(dev, corr, offset, e_mask, E, best_h)
    pose_h, angle_h = _prefilled_call(native_lib, *args, po.DISTANCE)
    assert [p["status"] for p in po.decode(pose_h)] == [po.OK, po.NO_VOTE, po.NOT_ESSENTIAL, po.NO_MODEL]
    assert np.isnan(angle_h[:n]).all() and np.isnan(angle_h[2 * n:]).all() and not np.isnan(angle_h[n:2 * n]).any()
    _assert_same_bits(pose_h, angle_h, *op.pair_poses(*args, po.DISTANCE))
    # the ragged call: pairs of 0 .. 1025 items, with and without a model
    ws = ragged["ws"]
    pose_h, angle_h = _prefilled_call(native_lib, ragged["corr_t"], ragged["offset_t"], ws.E, ws.e_result, ws.e_mask, ws.verdict,
                                      po.DISTANCE)
    _assert_same_bits(pose_h, angle_h, ws.pose, ws.angle)
    assert {p["status"] for p in po.decode(pose_h)} >= {po.OK, po.NO_MODEL}
    # a refused table: the verify call's own mark, then a hand-built one over a table that points far outside
    swapped = ragged["offset"].copy()
    swapped[8], swapped[9] = swapped[9], swapped[8]
    Q, N = len(vo.SIZES), len(ragged["corr"])
    bad = device.ViewGraphWorkspace(Q, N, 65, dev)
    swapped_t = device.to_device(swapped, torch.int64)
    bad.run(ragged["corr_t"], swapped_t, device.to_device(np.full(Q, 5.0)), THR, vo.RMS, MAX_RATIO, SEED)
    pose_h, angle_h = _prefilled_call(native_lib, ragged["corr_t"], swapped_t, bad.E, bad.e_result, bad.e_mask, bad.verdict,
                                      po.DISTANCE)
    for p in po.decode(pose_h):
        _assert_filler(p, po.BAD_OFFSETS)
    assert np.isnan(angle_h).all()
    corr, _, e_mask, R, t = po.edge_case_fixture()
    wild = np.array([0, 2**40, -2**40, len(corr)], dtype=np.int64)
    E = np.tile(po.essential(R, t).reshape(1, 9), (3, 1))
    args = _hand_built(dev, corr, wild, e_mask, E, np.zeros(3, np.int64), kind=vo.BAD_OFFSETS)
    pose_h, angle_h = _prefilled_call(native_lib, *args, po.DISTANCE)
    for p in po.decode(pose_h):
        _assert_filler(p, po.BAD_OFFSETS)
    assert np.isnan(angle_h).all()


def test_statuses_and_opcheck(dev, ragged):
    """no_model, not_essential, no_vote and ok side by side in one hand-built call; items no pair owns; the op under opcheck."""
    from structure_from_motion_amd import ops

    sc, n, corr, offset, e_mask, E, best_h = _four_statuses(dev)
    args = _hand_built(dev, corr, offset, e_mask, E, best_h)
    op = ops.load()
    pose_t, angle_t = op.pair_poses(*args, po.DISTANCE)
    pose, angle = po.decode(pose_t.cpu().numpy()), angle_t.cpu().numpy()
    assert pose[0]["status"] == po.OK and pose[0]["votes"][pose[0]["best"]] == n
    _assert_filler(pose[1], po.NO_VOTE)
    _assert_filler(pose[2], po.NOT_ESSENTIAL)
    _assert_filler(pose[3], po.NO_MODEL)
    assert not np.isnan(angle[n:2 * n]).any() and np.isnan(angle[:n]).all() and np.isnan(angle[2 * n:]).all()
    want = po.pair_pose(sc["corr"], np.ones(n, np.uint8), E[0].reshape(3, 3))
    assert abs(pose[0]["median_angle"] - want["median_angle"]) <= MEDIAN_ATOL
    # a best_h past the table is no model, not an index
    past = _hand_built(dev, corr, offset, e_mask, E, np.array([1, 7, 2**40, -5], dtype=np.int64))
    for p in po.decode(op.pair_poses(*past, po.DISTANCE)[0].cpu().numpy()):
        _assert_filler(p, po.NO_MODEL)
    # two calls, the same bits
    pose_2, angle_2 = op.pair_poses(*args, po.DISTANCE)
    assert torch.equal(pose_t, pose_2) and torch.equal(angle_t.view(torch.int64), angle_2.view(torch.int64))
    torch.library.opcheck(op.pair_poses.default, args + (po.DISTANCE,), test_utils=("test_schema", "test_faketensor"))
    # the ragged call's record is reproducible too
    ws = ragged["ws"]
    pose_r, angle_r = op.pair_poses(ragged["corr_t"], ragged["offset_t"], ws.E, ws.e_result, ws.e_mask, ws.verdict, po.DISTANCE)
    assert torch.equal(pose_r, ws.pose) and torch.equal(angle_r.view(torch.int64), ws.angle.view(torch.int64))


# What run(views=8, tracks="matches", verify="batched") returned before the seed pair could be chosen: every key and value,
# recorded on an MI355X from the app as it was (two runs gave the same digits; the route draws every sample from its seeds).
PARENT_FIRST = {
    "views": 8, "points": 2000, "views_registered": 8, "registration_order": [0, 1, 2, 3, 4, 5, 6, 7],
    "rotation_error_rad": {0: 0.0, 1: 0.00018724564624562968, 2: 0.00053489041897409, 3: 0.00046486449057054935,
                           4: 0.0006357770278601197, 5: 0.0008103705135069837, 6: 0.0008635758468838627,
                           7: 0.0010646944973317968},
    "translation_error": {0: 0.0, 1: 0.00313333723112794, 2: 0.005332556264782923, 3: 0.004219238721373442,
                          4: 0.004623532295682364, 5: 0.006361373260948744, 6: 0.006735652315937651, 7: 0.007867257598275081},
    "rms_px": 0.6081922694171563, "ba_observations": 11514, "ba_status": 0, "points_ok": 1968,
    "steps": [{"view": 1, "points_ok": 1194}, {"view": 2, "pnp_inliers": 972, "ba_status": 0, "points_ok": 1659},
              {"view": 3, "pnp_inliers": 1262, "ba_status": 0, "points_ok": 1816},
              {"view": 4, "pnp_inliers": 1310, "ba_status": 0, "points_ok": 1873},
              {"view": 5, "pnp_inliers": 1355, "ba_status": 0, "points_ok": 1906},
              {"view": 6, "pnp_inliers": 1352, "ba_status": 0, "points_ok": 1939},
              {"view": 7, "pnp_inliers": 1327, "ba_status": 0, "points_ok": 1968}],
    "track_build": {"tracks": 1971, "observations": 11648, "conflicts": 28, "unmatched": 3098, "components": 1999,
                    "pure_track_fraction": 0.9974632166412988, "pairs_kept": 18, "pairs_essential": 18, "pairs_homography": 0,
                    "pairs_none": 0},
}
PARENT_KEYS = set(PARENT_FIRST)
PARENT_RTOL = 1e-9   # the recorded figures are bit-exact on the device; this leaves room for the host's arc cosine and norms only


def _assert_same_values(got, want, where="out"):
    """Keys, counts and orders exactly; a float within PARENT_RTOL (an exact 0 stays one)."""
    if isinstance(want, dict):
        assert isinstance(got, dict) and set(got) == set(want), where
        for key in want:
            _assert_same_values(got[key], want[key], f"{where}[{key!r}]")
    elif isinstance(want, list):
        assert len(got) == len(want), where
        for k, (g, w) in enumerate(zip(got, want)):
            _assert_same_values(g, w, f"{where}[{k}]")
    elif isinstance(want, float):
        assert abs(float(got) - want) <= PARENT_RTOL * abs(want), (where, got, want)
    else:
        assert int(got) == want, (where, got, want)


def test_app_seed_pair_auto(dev):
    from apps import sfm_multi_view as app

    with pytest.raises(ValueError, match="seed_pair"):
        app.run(seed_pair="best")
    for kwargs in (dict(), dict(tracks="matches"), dict(verify="batched")):
        with pytest.raises(ValueError, match="needs tracks='matches' and verify='batched'"):
            app.run(seed_pair="auto", **kwargs)
    first = app.run(views=8, tracks="matches", verify="batched")
    auto = app.run(views=8, tracks="matches", verify="batched", seed_pair="auto", details=True)
    print("first", {k: first[k] for k in ("registration_order", "rotation_error_rad", "translation_error", "rms_px", "points_ok")})
    print("auto", {k: auto[k] for k in ("seed_pair", "median_angle_deg", "registration_order", "rotation_error_rad",
                                        "translation_error", "rms_px", "points_ok")})
    # the default route: the keys and the values it had, whether the new argument is left out or spelt
    _assert_same_values(first, PARENT_FIRST)
    _assert_same_values(app.run(views=8, tracks="matches", verify="batched", seed_pair="first", seed_min_angle_deg=5.0), PARENT_FIRST)
    assert first["registration_order"][:2] == [0, 1] and first["views_registered"] == 8
    assert set(auto) - {"_scene", "_status", "_graph"} == PARENT_KEYS | {"seed_pair", "median_angle_deg"}
    assert auto["views_registered"] == 8 and auto["registration_order"][:2] == auto["seed_pair"]
    assert auto["median_angle_deg"] >= 2.0
    graph = auto["_graph"]
    q_first = [tuple(p) for p in graph.pairs.tolist()].index((0, 1))
    q_auto = [tuple(p) for p in graph.pairs.tolist()].index(tuple(auto["seed_pair"]))
    print("median angle of (0, 1)", graph.pose.median_angle_deg[q_first], "status", graph.pose.status[q_first])
    assert auto["median_angle_deg"] == graph.pose.median_angle_deg[q_auto] and graph.pose.status[q_auto] == "ok"
    # views 0 and 1 are one 5-degree step apart with every point in front of both: the pair has a pose and an angle to compare
    assert graph.pose.status[q_first] == "ok" and np.isfinite(graph.pose.median_angle_deg[q_first])
    assert auto["median_angle_deg"] >= graph.pose.median_angle_deg[q_first]
    assert max(auto["rotation_error_rad"].values()) <= 2.0 * max(first["rotation_error_rad"].values())
    assert max(auto["translation_error"].values()) <= 2.0 * max(first["translation_error"].values())
