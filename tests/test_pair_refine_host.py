"""Host side of the refinement of every pair's relative pose: the exports and the record layout, the
argument checks of ``sfm_refine_pair_poses``, ``verify_pairs`` and ``refine_relative_poses``, the analytic Jacobian of the
NumPy definition against central differences, its identities, the accuracy condition on the oracle chain alone and the
margins and the spread the GPU comparisons rest on.  Nothing here needs a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pair_refine_cases as pc
import pair_refine_oracle as pr
import view_graph_pose_oracle as po
from geometry_cases import rotation
from structure_from_motion_amd.epipolar import view_graph as vg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = po.ho.synthetic.BENCH_K
EINVAL = -1   # SFM_EINVAL


def test_exports_layout_and_op_schema(native_lib):
    from structure_from_motion_amd import _native, build, device, ops

    assert "sfm_view_graph_refine.hip" in build.SOURCES
    assert _native.ABI_VERSION == 15 and native_lib.sfm_abi_version() == 15   # new symbols only
    with open(os.path.join(REPO, "include", "sfm_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint sfm_refine_pair_poses\s*\(", header)
    for code, name in enumerate(("OK", "NO_POSE", "TOO_FEW")):
        assert re.search(rf"#define SFM_PAIR_REFINE_{name} {code}\b", header)
    # the record: the header's fields in order, eight-byte fields first, 40 bytes
    body = re.search(r"typedef struct sfm_pair_refine_info \{(.*?)\} sfm_pair_refine_info;", header, re.S).group(1)
    fields = re.findall(r"^\s*(double|int32_t)\s+(\w+);", body, re.M)
    assert [name for _, name in fields] == [name for name, _ in _native.PairRefineInfo._fields_] == list(pr.INFO_DTYPE.names)
    assert [C.sizeof(ctype) for _, ctype in _native.PairRefineInfo._fields_] == [8 if kind == "double" else 4 for kind, _ in fields]
    assert "static_assert(sizeof(sfm_pair_refine_info) == 40" in header
    assert C.sizeof(_native.PairRefineInfo) == 40 == device.PAIR_REFINE_INFO_BYTES == pr.INFO_DTYPE.itemsize
    assert device.PAIR_REFINE_INFO_DTYPE == pr.INFO_DTYPE
    assert [(n, pr.INFO_DTYPE.fields[n][1]) for n in pr.INFO_DTYPE.names] == [
        (n, getattr(_native.PairRefineInfo, n).offset) for n, _ in _native.PairRefineInfo._fields_]
    assert device.PAIR_REFINE_STATUS == ("ok", "no_pose", "too_few") == pr.STATUS
    assert (device.PAIR_REFINE_OK, device.PAIR_REFINE_NO_POSE, device.PAIR_REFINE_TOO_FEW) == (pr.OK, pr.NO_POSE, pr.TOO_FEW)
    assert pc.POSE_DTYPE == device.POSE_DTYPE
    assert "sfm_refine_pair_poses" in _native.SIGNATURES and native_lib.sfm_refine_pair_poses is not None
    assert hasattr(device.ViewGraphWorkspace, "refine_poses")
    op = ops.load()
    # listed beside the two tuples that an earlier schema guard pins, and reached by the stream case all the same
    assert ops.LATER_FUNCTIONAL_OPS == ("refine_pair_poses",)
    assert not set(ops.LATER_FUNCTIONAL_OPS) & set(ops.FUNCTIONAL_OPS + ops.INPLACE_OPS)
    assert pc.stream_cases.CASES["refine_pair_poses"].entries == ("sfm_refine_pair_poses",)
    assert str(op.refine_pair_poses.default._schema) == (
        "sfm_hip::refine_pair_poses(Tensor corr, Tensor offset, Tensor pose, float thr, int aggregation, int rounds, "
        "int max_steps) -> (Tensor, Tensor, Tensor)")
    import lib.epipolar.view_graph as drop_in

    assert drop_in.refine_relative_poses is vg.refine_relative_poses and drop_in.PairRefinement is vg.PairRefinement
    assert vg.PairRefinement._fields == ("graph", "start_error", "error", "start_count", "count", "accepted", "lm_steps", "status",
                                         "inlier_matches")


def test_pinned_named_tuples_are_unchanged():
    assert vg.ViewGraph._fields == ("pairs", "kind", "E", "H", "essential_count", "homography_count", "ratio", "essential_inliers",
                                    "homography_inliers", "inlier_matches", "pose")
    assert vg.ViewGraph._fields[-1] == "pose" and vg.ViewGraph._field_defaults == {"pose": None}
    assert vg.PairPoses._fields == ("R", "t", "votes", "in_front", "median_angle_deg", "status")
    assert vg.PairPoses._field_defaults == {}


def test_meta_kernel_shapes():
    import torch

    from structure_from_motion_amd import ops

    op = ops.load()
    meta = lambda shape, dtype: torch.empty(shape, dtype=dtype, device="meta")   # noqa: E731
    pose, mask, info = op.refine_pair_poses(meta((100, 4), torch.float64), meta((4,), torch.int64), meta((3, 128), torch.uint8),
                                            6e-6, 3, 2, 20)
    assert pose.shape == (3, 128) and pose.dtype == torch.uint8 and mask.shape == (100,) and mask.dtype == torch.uint8
    assert info.shape == (3, 5) and info.dtype == torch.int64


def _call(lib, n_total=100, pairs=3, aggregation=3, rounds=2, max_steps=20, null=(), alias=False):
    """``sfm_refine_pair_poses`` with host addresses that a refused call never follows."""
    scratch = [(C.c_double * 16)() for _ in range(6)]
    p = {name: (None if name in null else C.addressof(buf))
         for name, buf in zip(("corr", "offset", "pose_in", "pose_out", "mask_out", "info"), scratch)}
    if alias:
        p["pose_out"] = p["pose_in"]
    return lib.sfm_refine_pair_poses(p["corr"], n_total, p["offset"], pairs, p["pose_in"], 6e-6, aggregation, rounds, max_steps,
                                     p["pose_out"], p["mask_out"], p["info"], None)


def test_entry_refuses_bad_arguments_before_any_launch(native_lib):
    lib = native_lib
    for kwargs in (dict(n_total=-1), dict(pairs=-1), dict(pairs=65536), dict(n_total=2**31), dict(rounds=-1), dict(max_steps=-1),
                   dict(aggregation=-1), dict(aggregation=4), dict(alias=True)):
        assert _call(lib, **kwargs) == EINVAL, kwargs
    assert _call(lib, pairs=65536) == EINVAL and b"65535" in lib.sfm_last_error()
    assert _call(lib, n_total=2**31) == EINVAL and b"2^31" in lib.sfm_last_error()
    assert _call(lib, aggregation=4) == EINVAL and b"aggregation" in lib.sfm_last_error()
    assert _call(lib, alias=True) == EINVAL and b"alias" in lib.sfm_last_error()
    for name in ("corr", "offset", "pose_in", "pose_out", "mask_out", "info"):
        assert _call(lib, null=(name,)) == EINVAL and b"null pointer" in lib.sfm_last_error(), name
    assert _call(lib, pairs=0) == 0                                    # no pairs: a no-op
    assert _call(lib, pairs=0, null=("corr", "offset", "pose_in")) == 0


def _graph(sizes=(10, 12)):
    rng = np.random.default_rng(3)
    features, pairs, matches = [], [], []
    for q, n in enumerate(sizes):
        features += [rng.uniform(0, 600, (n, 2)), rng.uniform(0, 600, (n, 2))]
        pairs.append((2 * q, 2 * q + 1))
        matches.append(np.column_stack([np.arange(n), np.arange(n)]))
    return features, pairs, matches


def _no_device(monkeypatch):
    from structure_from_motion_amd import device

    def no_device(*args, **kwargs):
        raise AssertionError("device touched")

    monkeypatch.setattr(device, "require_gpu", no_device)
    monkeypatch.setattr(device, "to_device", no_device)
    monkeypatch.setattr(device, "refine_pair_poses", no_device)


def _posed_graph(Q, pose=True):
    none = np.full((Q, 3, 3), np.nan)
    poses = vg.PairPoses(np.tile(np.eye(3), (Q, 1, 1)), np.tile([1.0, 0.0, 0.0], (Q, 1)), np.zeros((Q, 4), np.int64),
                         np.zeros(Q, np.int64), np.zeros(Q), ["ok"] * Q)
    pairs = np.array([(2 * q, 2 * q + 1) for q in range(Q)], dtype=np.int64).reshape(Q, 2)
    return vg.ViewGraph(pairs, ["essential"] * Q, none, none.copy(), np.zeros(Q, np.int64), np.zeros(Q, np.int64), np.zeros(Q),
                        [None] * Q, [None] * Q, [None] * Q, poses if pose else None)


def test_arguments_are_checked_before_device_work(monkeypatch):
    _no_device(monkeypatch)
    features, pairs, matches = _graph()
    with pytest.raises(ValueError, match="relative_pose=True"):
        vg.verify_pairs(K, features, pairs, matches, 2e-5, refine_pose_rounds=1)
    with pytest.raises(ValueError, match="relative_pose=True"):
        vg.verify_pairs(K, features, [], [], 2e-5, refine_pose_rounds=2)
    for bad in (-1, 1.5, "2", None, True, 2**31):
        with pytest.raises(ValueError, match="rounds"):
            vg.verify_pairs(K, features, pairs, matches, 2e-5, relative_pose=True, refine_pose_rounds=bad)
        with pytest.raises(ValueError, match="max_steps"):
            vg.verify_pairs(K, features, pairs, matches, 2e-5, relative_pose=True, refine_pose_rounds=1, refine_pose_max_steps=bad)
        with pytest.raises(ValueError, match="rounds"):
            vg.refine_relative_poses(K, features, _posed_graph(2), matches, 2e-5, rounds=bad)
        with pytest.raises(ValueError, match="max_steps"):
            vg.refine_relative_poses(K, features, _posed_graph(2), matches, 2e-5, max_steps=bad)
    # the defaults leave the feature off: an empty graph needs no device with them or with explicit zeros
    assert vg.verify_pairs(K, features, [], [], 2e-5, relative_pose=True, refine_pose_rounds=0).pose.status == []
    with pytest.raises(ValueError, match="graph.pose"):
        vg.refine_relative_poses(K, features, _posed_graph(2, pose=False), matches, 2e-5)
    with pytest.raises(ValueError, match="one entry per pair"):
        vg.refine_relative_poses(K, features, _posed_graph(2), matches[:1], 2e-5)
    with pytest.raises(ValueError, match="inlier_threshold"):
        vg.refine_relative_poses(K, features, _posed_graph(2), matches, float("nan"))
    short = _posed_graph(2)
    short = short._replace(pose=short.pose._replace(status=["ok"]))
    with pytest.raises(ValueError, match="one pose per pair"):
        vg.refine_relative_poses(K, features, short, matches, 2e-5)
    odd = _posed_graph(2)
    odd = odd._replace(pose=odd.pose._replace(status=["ok", "fine"]))
    with pytest.raises(ValueError, match="unknown names"):
        vg.refine_relative_poses(K, features, odd, matches, 2e-5)
    with pytest.raises(ValueError, match="camera"):
        vg.refine_relative_poses(np.eye(2), features, _posed_graph(2), matches, 2e-5)
    empty = vg.refine_relative_poses(K, features, _posed_graph(0), [], 2e-5)
    assert empty.status == [] and empty.inlier_matches == [] and len(empty.count) == 0


# general, the forward motion (|t_0| = |t_1| = 0: the tie of the basis rule), and a translation within 1e-9 of an axis
JACOBIAN_T = {"general": np.array([0.5, 0.05, 0.1]), "tz": np.array([0.0, 0.0, 1.0]), "near_axis": np.array([1.0, 1e-9, -2e-9])}


@pytest.mark.parametrize("name", sorted(JACOBIAN_T))
def test_analytic_jacobian_matches_central_differences(name):
    t = JACOBIAN_T[name] / np.linalg.norm(JACOBIAN_T[name])
    R = rotation((1.0, 2.0, 3.0), 12.0)
    sc = po.ho.scene(R, t, False, 40, 5, 0.5)
    R0, t0 = pc.perturbed(R, t, 0.05, 3) if name != "tz" else (pc.perturbed(R, t, 0.05, 3)[0], t)
    b1, b2 = pr.tangent_basis(t0)
    assert abs(b1 @ t0) < 1e-15 and abs(b2 @ t0) < 1e-15 and abs(b1 @ b2) < 1e-15
    assert np.allclose([b1 @ b1, b2 @ b2], 1.0, atol=1e-15) and np.allclose(np.cross(b1, b2), t0, atol=1e-15)
    if name == "tz":
        assert np.array_equal(b1, [0.0, 1.0, 0.0]) and np.array_equal(b2, [-1.0, 0.0, 0.0])   # e = x, the first of the tie
    res, J = pr.residuals_and_jacobian(R0, t0, sc["corr"])
    assert np.allclose((res * res).sum(axis=1), po.orc.sed_values(pr.essential(R0, t0), sc["corr"]), rtol=1e-12, atol=0.0)
    # central differences with h = 1e-6: truncation h^2 |J'''| ~ 1e-12 |J|, rounding eps |res| / h ~ 1e-13; bound 1e-7 |J|
    h = 1e-6
    for k in range(pr.UNKNOWNS):
        d = np.zeros(pr.UNKNOWNS)
        d[k] = h
        plus = pr.residuals_and_jacobian(*pr.apply_step(R0, t0, d), sc["corr"])[0]
        minus = pr.residuals_and_jacobian(*pr.apply_step(R0, t0, -d), sc["corr"])[0]
        numeric = (plus - minus) / (2.0 * h)
        assert np.abs(numeric - J[:, :, k]).max() <= 1e-7 * np.abs(J[:, :, k]).max(), (name, k)
    # and H, g are the sums of the same Jacobian
    H, g, cost = pr.system(R0, t0, sc["corr"])
    assert np.allclose(H, np.einsum("mri,mrj->ij", J, J), rtol=1e-13) and np.allclose(g, np.einsum("mri,mr->i", J, res), rtol=1e-12)
    assert np.isclose(cost, (res * res).sum(), rtol=1e-12)


def test_zero_rounds_and_zero_steps_are_identities():
    corr, offset, table = pc.fixture()
    poses = pc.pose_dicts(table)
    start, start_mask = pr.refine_pairs(corr, offset, poses, pc.THR, pr.RMS, rounds=0, max_steps=20)
    still, still_mask = pr.refine_pairs(corr, offset, poses, pc.THR, pr.RMS, rounds=2, max_steps=0)
    assert np.array_equal(start_mask, still_mask)
    for q, (p, a, b) in enumerate(zip(poses, start, still)):
        for r in (a, b):
            assert np.array_equal(r["R"], p["R"], equal_nan=True) and np.array_equal(r["t"], p["t"], equal_nan=True)
            assert r["accepted"] == 0 and r["lm_steps"] == 0 and r["count"] == r["start_count"]
            assert np.array_equal(r["error"], r["start_error"], equal_nan=True)
        assert a["status"] == b["status"] and a["start_count"] == b["start_count"]
        lo, hi = offset[q], offset[q + 1]
        assert start_mask[lo:hi].sum() == a["count"]
    assert [r["status"] for r in start] == [pr.TOO_FEW, pr.TOO_FEW] + [pr.OK] * 2 + [pr.NO_POSE] + [pr.OK] * 8
    assert start_mask[offset[4]:offset[5]].sum() == 0 and start_mask[offset[10] + 7] == 0   # no pose; the NaN item


def test_oracle_statuses_and_special_pairs():
    res, mask, _, _ = pc.oracle_runs()[(2, 4, pr.RMS)]
    corr, offset, table = pc.fixture()
    by = dict(zip(pc.NAMES, res))
    assert by["empty"]["status"] == pr.TOO_FEW and by["five"]["status"] == pr.TOO_FEW and by["five"]["count"] == 5
    assert by["no_model"]["status"] == pr.NO_POSE
    for name in ("true_pose", "repeated"):   # nothing to gain; a rank-deficient H
        q = pc.NAMES.index(name)
        assert by[name]["accepted"] == 0 and np.array_equal(by[name]["R"], table[q]["R"]) and np.array_equal(by[name]["t"], table[q]["t"])
    assert by["repeated"]["lm_steps"] == 0 and by["repeated"]["count"] == 300
    for name in ("six", "n255", "n256", "n257", "n1025", "nan_item", "tz", "pan"):
        assert by[name]["accepted"] >= 1 and by[name]["status"] == pr.OK, name
        assert by[name]["count"] >= by[name]["start_count"]
    assert abs(np.linalg.norm(by["tz"]["t"]) - 1.0) < 1e-15 and not np.array_equal(by["tz"]["t"], [0.0, 0.0, 1.0])


def test_parity_cases_keep_their_margins_and_the_spread_is_as_recorded():
    """What the GPU comparisons rest on, for every compared pair of every run: no re-scored item within 1e-6 relative of the
    threshold, every accept test decided by 1e-10 of the cost, and the spread between the two item orders within SPREAD."""
    runs = pc.oracle_runs()
    spread = dict(R=0.0, t=0.0, error=0.0)
    least_thr = least_accept = np.inf
    for rounds, steps, agg, names in pc.PARITY_RUNS:
        res, _, rev, traces = runs[(rounds, steps, agg)]
        for q in pc.compared(names):
            a, b, trace = res[q], rev[q], traces.get(q, {})
            least_thr = min(least_thr, pr.threshold_margin(trace, pc.THR))
            least_accept = min(least_accept, pr.accept_margin(trace))
            assert pr.threshold_margin(trace, pc.THR) >= pc.MIN_THRESHOLD_MARGIN, (rounds, steps, pc.NAMES[q])
            assert pr.accept_margin(trace) >= pc.MIN_ACCEPT_MARGIN, (rounds, steps, pc.NAMES[q])
            assert all(a[k] == b[k] for k in ("start_count", "count", "accepted", "lm_steps", "status"))
            if a["status"] == pr.NO_POSE:
                continue
            spread["R"] = max(spread["R"], np.abs(a["R"] - b["R"]).max())
            spread["t"] = max(spread["t"], np.abs(a["t"] - b["t"]).max())
            for k in ("start_error", "error"):
                if a["count"] and a[k]:
                    spread["error"] = max(spread["error"], abs(a[k] - b[k]) / a[k])
    print("spread between item orders:", spread, "least threshold margin:", least_thr, "least accept margin:", least_accept)
    for k, v in spread.items():
        assert v <= pc.SPREAD[k], (k, v)
        assert v >= 0.1 * pc.SPREAD[k], (k, v)   # the recorded figure is the measured one, not a generous one
    # every run takes LM steps somewhere, and the four-step run takes four
    assert max(r["lm_steps"] for r in runs[(2, 4, pr.RMS)][0]) >= 4


def test_accuracy_condition_on_the_oracle_chain():
    """The chain five_point.fit_corr on the Philox samples -> six-item selection -> pose oracle -> refine oracle, on the twelve
    pairs of the feature test: both medians strictly lower after refinement, at most four pairs worse in either measure."""
    scenes = pc.accuracy_scenes()
    start = [pc.oracle_chain(sc, pc.ACCURACY_SEED + q) for q, sc in enumerate(scenes)]
    assert all(p["status"] == po.OK for p in start)
    refined = [pr.refine(sc["corr"], p["R"], p["t"], pc.THR, pr.RMS, rounds=2, max_steps=20) for sc, p in zip(scenes, start)]
    before = pc.pose_errors([p["R"] for p in start], [p["t"] for p in start], scenes)
    after = pc.pose_errors([r["R"] for r in refined], [r["t"] for r in refined], scenes)
    s = pc.accuracy_summary(before, after)
    print("oracle chain: median rotation / direction error in degrees before", s["median_before"], "after", s["median_after"],
          "pairs worse in either measure:", s["worse"], "LM steps:", [r["lm_steps"] for r in refined])
    assert (s["median_after"] < s["median_before"]).all()
    assert s["worse"] <= pc.MAX_WORSE
    assert all(r["accepted"] >= 1 for r in refined)


def test_app_refuses_refine_pairs_off_the_batched_route(monkeypatch):
    _no_device(monkeypatch)
    from apps import sfm_multi_view

    with pytest.raises(ValueError, match="refine_pairs needs"):
        sfm_multi_view.run(refine_pairs=2)
    with pytest.raises(ValueError, match="refine_pairs needs"):
        sfm_multi_view.run(tracks="matches", verify="loop", refine_pairs=1)
    for bad in (-1, 1.5, True, None):
        with pytest.raises(ValueError, match="refine_pairs must be"):
            sfm_multi_view.run(tracks="matches", verify="batched", refine_pairs=bad)
