"""The ragged similarity alignment without a GPU: the declaration and the bindings, every refusal of the C entry
point before a launch, the checks of ``align_models`` before any device work, the items of a pair, ``merge_frames`` on hand-made
alignments, the oracle's own result on the fixture and the stream case."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import align_models_cases as cases
import similarity_cases as sc
import similarity_oracle as so
from structure_from_motion_amd import _native
from structure_from_motion_amd.multiview import alignment as al

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SFM_EINVAL = -1   # include/sfm_hip.h


def _no_device(monkeypatch):
    from structure_from_motion_amd import device

    def no_device(*args, **kwargs):
        raise AssertionError("device touched")

    monkeypatch.setattr(device, "require_gpu", no_device)
    monkeypatch.setattr(device, "to_device", no_device)


def test_entry_point_signature_and_header(native_lib):
    with open(os.path.join(REPO, "include", "sfm_hip.h")) as f:
        header = f.read()

    def ctype_of(p):
        if "*" in p:
            return C.c_void_p
        return {"uint64_t": C.c_uint64, "int64_t": C.c_int64, "double": C.c_double, "int": C.c_int}[p.split()[0]]
    m = re.search(r"\bint sfm_align_models\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m is not None
    params = [p.strip() for p in " ".join(m.group(1).split()).split(",")]
    sig = _native.SIGNATURES["sfm_align_models"]
    assert len(params) == len(sig) == 28 and params[-1] == "void* stream"
    assert [ctype_of(p) for p in params] == list(sig)
    assert [p.split()[-1].lstrip("*") for p in params[:13]] == ["seed", "seed_stride", "h_begin", "pairs", "n_total", "offset", "pair_count",
                                                                 "max_items", "thr", "min_extra", "h_count", "aggregation", "refine_rounds"]
    assert [p.split()[-1].lstrip("*") for p in params[13:]] == list(cases.BUFFER_NAMES) + ["workspace", "workspace_bytes", "stream"]
    m = re.search(r"\bint64_t sfm_align_models_workspace_bytes\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m is not None and [ctype_of(p.strip()) for p in m.group(1).split(",")] == [C.c_int64] * 3
    assert "sfm_align_models_workspace_bytes" in _native.OTHER_SYMBOLS
    for code, name in enumerate(("OK", "NO_MODEL", "TOO_FEW", "BAD_OFFSETS")):
        assert re.search(rf"#define SFM_ALIGN_{name} {code}\b", header)
    assert re.search(r"#define SFM_ABI_VERSION 15\b", header)
    assert native_lib.sfm_align_models is not None and native_lib.sfm_abi_version() == 15 == _native.ABI_VERSION
    from structure_from_motion_amd import build, device

    assert "sfm_align_models.hip" in build.SOURCES
    assert {"sfm_similarity.h", "sfm_similarity_reduce.h"} <= set(build.HEADERS)
    assert _native.ALIGN_STATUS == ("ok", "no_model", "too_few", "bad_offsets") == device.ALIGN_STATUS == cases.STATUS
    assert (device.ALIGN_OK, device.ALIGN_NO_MODEL, device.ALIGN_TOO_FEW, device.ALIGN_BAD_OFFSETS) == (0, 1, 2, 3)
    assert hasattr(device.AlignModelsWorkspace, "buffers") and hasattr(device.AlignModelsWorkspace, "run")
    assert callable(device.read_align_status)


def test_entry_point_refuses_bad_arguments_before_any_launch(native_lib):
    """Every refusal is an SFM_EINVAL with its reason, checked on the host: no GPU is needed to be refused."""
    lib = native_lib
    p = C.c_void_p(0x1000)   # never dereferenced: the call is refused first
    odd = C.c_void_p(0x1008)

    def call(seed=1, stride=1, h_begin=0, pairs=p, n=10, offset=p, Q=2, most=10, thr=p, gate=p, h=8, agg=3, rounds=2, S=p, mask=p,
             mask_out=C.c_void_p(0x2000), status=p, ws=p, ws_bytes=1 << 30):
        return lib.sfm_align_models(seed, stride, h_begin, pairs, n, offset, Q, most, thr, gate, h, agg, rounds, S, p, p, p, p, p, p, mask,
                                    p, mask_out, p, status, ws, ws_bytes, None)

    def refused(reason, **kw):
        assert call(**kw) == SFM_EINVAL, kw
        assert reason in lib.sfm_last_error(), (reason, lib.sfm_last_error())
    refused(b"negative size", n=-1, most=0)
    refused(b"negative size", Q=-1)
    refused(b"negative size", rounds=-1)
    refused(b"negative size", most=-1)
    refused(b"2^31", n=2**31)
    refused(b"65535", Q=65536)
    refused(b"max_items", most=11)
    refused(b"at least one hypothesis", h=0)
    refused(b"at least one hypothesis", h=-3)
    refused(b"one launch covers", h=2**40)
    refused(b"unknown aggregation", agg=4)
    refused(b"unknown aggregation", agg=-1)
    refused(b"h_begin", h_begin=-1)
    refused(b"null pointer", offset=None)
    refused(b"null pointer", thr=None)
    refused(b"null pointer", gate=None)
    refused(b"null pointer", S=None)
    refused(b"null pointer", status=None)
    refused(b"null pointer", pairs=None)
    refused(b"null pointer", mask=None)
    refused(b"null pointer", ws=None)
    refused(b"16-byte aligned", pairs=odd)
    refused(b"16-byte aligned", ws=odd)
    refused(b"alias", mask_out=p)
    refused(b"workspace too small", ws_bytes=lib.sfm_align_models_workspace_bytes(10, 2, 10) - 1)
    refused(b"workspace too small", ws_bytes=0)
    assert call(Q=0) == _native.SFM_OK                       # a no-op
    assert call(Q=0, offset=None, ws=None) == _native.SFM_OK
    assert call(n=2**31 - 1, most=0, Q=0) == _native.SFM_OK   # the largest item count


def test_workspace_bytes(native_lib):
    size = native_lib.sfm_align_models_workspace_bytes
    for n, Q, most in ((-1, 1, 0), (2**31, 1, 10), (10, -1, 10), (10, 65536, 10), (10, 1, -1), (10, 1, 11)):
        assert size(n, Q, most) == -1, (n, Q, most)
    assert size(0, 0, 0) >= 0 and size(2**31 - 1, 65535, 2**31 - 1) > 0
    # one partial record per 2 048 items of the largest pair, 128 at the most; it grows with the pairs
    assert size(10**6, 3, 2048) < size(10**6, 3, 2049) < size(10**6, 3, 262144) == size(10**6, 3, 10**6)
    assert size(10**6, 3, 2049) < size(10**6, 30, 2049)   # (the pieces are rounded up to 256 bytes)


def test_ops_are_registered(native_lib):
    import torch

    from structure_from_motion_amd import ops

    op = ops.load()
    assert ops.ALIGN_MODELS_OPS == ("align_models", "align_models_")
    others = ops.FUNCTIONAL_OPS + ops.INPLACE_OPS + ops.LATER_FUNCTIONAL_OPS + ops.REGISTER_VIEWS_OPS + ops.SIMILARITY_OPS
    assert not set(ops.ALIGN_MODELS_OPS) & set(others)
    schema = str(op.align_models.default._schema)
    assert schema == ("sfm_hip::align_models(Tensor pairs, Tensor offset, Tensor thr, Tensor min_extra, int max_items, int seed, "
                      "int seed_stride, int h_begin, int h, int aggregation, int refine_rounds) -> "
                      "(Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
    schema = str(op.align_models_.default._schema)
    assert "Tensor(a!) S, Tensor(b!) model" in schema and "Tensor(l!) status) -> ()" in schema and "int h," not in schema
    meta = dict(device="meta")
    Q, N, h = 5, 700, 33
    pairs, offset = torch.empty((N, 6), dtype=torch.float64, **meta), torch.empty((Q + 1,), dtype=torch.int64, **meta)
    per_pair = torch.empty((Q,), dtype=torch.float64, **meta)
    model, mask_out, info, status, mask, result = op.align_models(pairs, offset, per_pair, per_pair, 300, 1, 1, 0, h, 3, 2)
    assert model.shape == (Q, 13) and model.dtype == torch.float64 and model.device.type == "meta"
    assert mask_out.shape == (N,) == mask.shape and mask.dtype == torch.uint8 == mask_out.dtype
    assert info.shape == (Q, 3) and info.dtype == torch.int64 and status.shape == (Q,) and status.dtype == torch.int32
    assert result.shape == (Q, 5) and result.dtype == torch.int64


# ---- align_models: the checks before any device work, and the items of a pair ------------------------------------------------
def _valid():
    rng = np.random.default_rng(3)
    points = [rng.normal(size=(6, 3)), rng.normal(size=(5, 3)), rng.normal(size=(4, 3))]
    ids = [np.array([9, 3, 7, 1, 5, 11]), np.array([5, 2, 9, 7, 1]), np.array([1, 2, 3, 4])]
    return dict(points=points, point_ids=ids, pairs=np.array([[0, 1], [2, 0]]), inlier_threshold=1e-6)


@pytest.mark.parametrize("change", [
    dict(points=[np.zeros((6, 2)), np.zeros((5, 3)), np.zeros((4, 3))]),
    dict(points=[np.zeros(18), np.zeros((5, 3)), np.zeros((4, 3))]),
    dict(points=[np.full((6, 3), np.nan), np.zeros((5, 3)), np.zeros((4, 3))]),
    dict(points=[np.full((6, 3), np.inf), np.zeros((5, 3)), np.zeros((4, 3))]),
    dict(points=[np.zeros((6, 3)), np.zeros((5, 3))]),                                               # one model short
    dict(point_ids=[np.arange(6), np.arange(5), np.arange(5)]),                                      # lengths differ
    dict(point_ids=[np.arange(6.0), np.arange(5), np.arange(4)]),                                    # floats
    dict(point_ids=[np.arange(6).reshape(6, 1), np.arange(5), np.arange(4)]),
    dict(point_ids=[np.array([0, 1, 2, 3, 4, 0]), np.arange(5), np.arange(4)]),                      # an id repeated within a model
    dict(pairs=np.array([[0, 0]])),                                                                  # i == j
    dict(pairs=np.array([[0, 3]])),                                                                  # outside the models
    dict(pairs=np.array([[-1, 1]])),
    dict(pairs=np.array([0, 1])),
    dict(pairs=np.array([[0.0, 1.0]])),
    dict(inlier_threshold=float("nan")),
    dict(inlier_threshold=np.array([1e-6, np.nan])),
    dict(inlier_threshold=np.array([1e-6, 1e-6, 1e-6])),                                             # one per pair means two
    dict(iterations=True),
    dict(iterations=10.0),
    dict(refine_rounds=True),
    dict(refine_rounds=-1),
    dict(seed=True),
    dict(seed=1.5),
    dict(min_num_extra_inliers=1.5),
    dict(min_num_extra_inliers=np.zeros(3, dtype=np.int64)),
    dict(min_extra_fraction=-0.1),
    dict(error_aggregation="rms"),
    dict(max_hypotheses_per_call=0),
    dict(max_hypotheses_per_call=True),
])
def test_arguments_are_checked_before_device_work(monkeypatch, change):
    _no_device(monkeypatch)
    args = _valid()
    args.update(change)
    with pytest.raises(ValueError):
        al.align_models(**args)


def test_no_pairs_and_no_iterations_need_no_device(monkeypatch):
    _no_device(monkeypatch)
    args = _valid()
    out = al.align_models(args["points"], args["point_ids"], np.zeros((0, 2), dtype=np.int64), 1e-6)
    assert out.status == [] and out.R.shape == (0, 3, 3) and out.inliers == [] and len(out.scale) == 0
    out = al.align_models(**args, iterations=0)
    assert out.status == ["no_model", "too_few"] and np.isnan(out.scale).all() and out.estimate(0) is None and out.estimate(1) is None
    assert out.common_count.tolist() == [4, 2] and out.inlier_count.tolist() == [0, 0] and np.all(out.error == np.inf)


def test_items_of_a_pair():
    """The common ids ascending, side A from model i and side B from model j, whatever the order of the ids in either model."""
    args = _valid()
    points, ids, pairs = args["points"], args["point_ids"], args["pairs"]
    items = al.common_items(ids, pairs)
    assert [c.tolist() for c, _, _ in items] == [[1, 5, 7, 9], [1, 3]]
    for (i, j), (common, at_i, at_j) in zip(pairs.tolist(), items):
        assert np.array_equal(common, np.intersect1d(ids[i], ids[j])) and np.all(np.diff(common) > 0)
        assert np.array_equal(ids[i][at_i], common) and np.array_equal(ids[j][at_j], common)
    # pair (2, 0): side A is model 2
    common, at_a, at_b = items[1]
    assert np.array_equal(points[2][at_a], points[2][[0, 2]]) and np.array_equal(points[0][at_b], points[0][[3, 1]])
    assert al.common_items(ids, np.zeros((0, 2), dtype=np.int64)) == []
    disjoint = al.common_items([np.array([1, 2]), np.array([3, 4])], np.array([[0, 1]]))[0]
    assert all(len(a) == 0 for a in disjoint)


# ---- merge_frames ---------------------------------------------------------------------------------------------------------------
# The largest disagreement of a tree pair over the hand-made inputs below, measured (these tests print it): 4.02e-15 degrees,
# 1.11e-16 in |log| of the scale ratio and 1.90e-15 units of distance — compositions of up to three similarities with translations
# of up to 3 units, within the 100 ulp (2.2e-14 relative, 1.3e-12 degrees) that round-off may take.  The tests assert ten times
# the measured values.
TREE_ROTATION_DEG, TREE_LOG_SCALE, TREE_DISTANCE = 10 * 4.02e-15, 10 * 1.11e-16, 10 * 1.90e-15
_TREE_WORST = [0.0, 0.0, 0.0]


def _frames_of(truth):
    """truth[k] = (s, R, t) mapping model k into the world; -> S(i, j), the exact alignment of model i onto model j."""
    def S(i, j):
        return al.compose(al.invert(truth[j]), truth[i])
    return S


def _check_tree(frames, pairs):
    for q in frames.tree_pairs.tolist():
        got = (frames.rotation_deg[q], frames.log_scale[q], frames.distance[q])
        assert all(np.isfinite(got)), (q, got)
        for k in range(3):
            _TREE_WORST[k] = max(_TREE_WORST[k], float(got[k]))
        assert got[0] <= TREE_ROTATION_DEG and got[1] <= TREE_LOG_SCALE and got[2] <= TREE_DISTANCE, (q, got)


def _assert_frames(frames, truth, root, reached):
    """G_k is truth[root]^-1 o truth[k] for every reached model."""
    assert frames.reached.tolist() == reached
    for k, ok in enumerate(reached):
        if not ok:
            assert np.isnan(frames.scale[k]) and np.isnan(frames.R[k]).all() and np.isnan(frames.t[k]).all()
            continue
        s, R, t = al.compose(al.invert(truth[root]), truth[k])
        assert abs(frames.scale[k] - s) <= 1e-13 * s and np.max(np.abs(frames.R[k] - R)) <= 1e-13, k
        assert np.max(np.abs(frames.t[k] - t)) <= 1e-12, k


TRUTH = [sc.similarity(50 + k) for k in range(5)]
CENTROIDS = np.random.default_rng(8).uniform(-1.0, 1.0, size=(8, 3))


def test_merge_frames_chain_reversed_edge_and_root():
    S = _frames_of(TRUTH)
    pairs = np.array([[0, 1], [2, 1], [2, 3]])   # the middle edge is reversed: it maps 2 onto 1
    found = cases.alignments([S(i, j) for i, j in pairs.tolist()], [50, 40, 30], CENTROIDS[:3])
    for root in (0, 3, 1):
        frames = al.merge_frames(4, pairs, found, root=root)
        _assert_frames(frames, TRUTH, root, [True] * 4)
        assert sorted(frames.tree_pairs.tolist()) == [0, 1, 2] and frames.usable.all()
        _check_tree(frames, pairs)
        assert len(al.inconsistent_alignments(frames, 1e-6, 1e-9)) == 0
        assert frames.scale[root] == 1.0 and np.array_equal(frames.R[root], np.eye(3)) and not frames.t[root].any()
    print("largest tree disagreement so far (deg, log scale, distance):", _TREE_WORST)


def test_merge_frames_loop_with_one_wrong_pair():
    """A square 0-1-2-3-0 and a diagonal; the pair with the fewest inliers is wrong (2 degrees, 1 % in scale): the tree avoids
    it, and it is the one pair that inconsistent_alignments names."""
    S = _frames_of(TRUTH)
    pairs = np.array([[0, 1], [1, 2], [2, 3], [3, 0], [0, 2]])
    sims = [S(i, j) for i, j in pairs.tolist()]
    wrong = 3
    s, R, t = sims[wrong]
    sims[wrong] = (1.01 * s, sc.rotation((0.0, 0.0, 1.0), 2.0) @ R, t + 0.05)
    found = cases.alignments(sims, [80, 70, 60, 20, 90], CENTROIDS[:5])
    frames = al.merge_frames(4, pairs, found)
    assert frames.tree_pairs.tolist() == [4, 0, 2]   # heaviest first; pair 1 would close the triangle 0-1-2
    assert wrong not in frames.tree_pairs.tolist()
    _assert_frames(frames, TRUTH, 0, [True] * 4)
    _check_tree(frames, pairs)
    assert al.inconsistent_alignments(frames, 0.5, 5e-3).tolist() == [wrong]
    assert abs(frames.rotation_deg[wrong] - 2.0) < 1e-9 and abs(frames.log_scale[wrong] - np.log(1.01)) < 1e-12
    assert frames.distance[wrong] > 1e-3
    # the loop pairs that are right close to round-off as well
    others = [q for q in range(5) if q != wrong and q not in frames.tree_pairs.tolist()]
    assert others and all(frames.rotation_deg[q] < 1e-11 and frames.log_scale[q] < 1e-13 for q in others)
    print("largest tree disagreement so far (deg, log scale, distance):", _TREE_WORST)


def test_merge_frames_unreached_model_and_unusable_pairs():
    S = _frames_of(TRUTH)
    pairs = np.array([[0, 1], [1, 2], [3, 4], [2, 3], [0, 4]])
    sims = [S(i, j) for i, j in pairs.tolist()]
    # pair 3 has too few inliers and pair 4 no model: 3 and 4 hang together, away from the root
    found = cases.alignments(sims, [50, 40, 30, 2, 0], CENTROIDS[:5], status=["ok", "ok", "ok", "ok", "no_model"])
    found.scale[4], found.R[4], found.t[4] = np.nan, np.nan, np.nan
    frames = al.merge_frames(5, pairs, found, min_inliers=3)
    assert frames.usable.tolist() == [True, True, True, False, False]
    _assert_frames(frames, TRUTH, 0, [True, True, True, False, False])
    assert sorted(frames.tree_pairs.tolist()) == [0, 1, 2]          # a forest: pair 2 joins the two unreached models
    _check_tree(al.merge_frames(5, pairs, found, min_inliers=2), pairs)
    assert np.isnan(frames.rotation_deg[[2, 3, 4]]).all() and np.isfinite(frames.rotation_deg[[0, 1]]).all()
    assert len(al.inconsistent_alignments(frames, 1e-6, 1e-9)) == 0
    frames = al.merge_frames(5, pairs, found, root=4)
    _assert_frames(frames, TRUTH, 4, [False, False, False, True, True])
    frames = al.merge_frames(5, pairs, found, min_inliers=2)          # pair 3 is usable now
    _assert_frames(frames, TRUTH, 0, [True] * 5)
    for bad in (dict(root=5), dict(root=-1), dict(root=True), dict(min_inliers=-1)):
        with pytest.raises(ValueError):
            al.merge_frames(5, pairs, found, **bad)
    with pytest.raises(ValueError):
        al.merge_frames(5, pairs[:4], found)


def test_merge_frames_ties_go_to_the_lower_pair_index():
    """A triangle of equal weights, one of its pairs wrong: Kruskal takes pairs 0 and 1, whichever of the three is wrong."""
    S = _frames_of(TRUTH)
    pairs = np.array([[0, 1], [1, 2], [0, 2]])
    for wrong in range(3):
        sims = [S(i, j) for i, j in pairs.tolist()]
        s, R, t = sims[wrong]
        sims[wrong] = (s, sc.rotation((1.0, 0.0, 0.0), 5.0) @ R, t)
        frames = al.merge_frames(3, pairs, cases.alignments(sims, [25, 25, 25], CENTROIDS[:3]))
        assert frames.tree_pairs.tolist() == [0, 1], wrong
        _check_tree(frames, pairs)
        assert al.inconsistent_alignments(frames, 0.5, 5e-3).tolist() == [2]
        assert abs(frames.rotation_deg[2] - 5.0) < 1e-9
    print("largest tree disagreement so far (deg, log scale, distance):", _TREE_WORST)


# ---- the oracle's own result on the fixture -------------------------------------------------------------------------------------
def test_the_oracles_winner_finds_the_clean_items_of_the_fixture():
    """With the oracle alone: per pair of the fixture with a winner, the oracle's pass and refit leave no displaced item among the
    inliers and at least 99 % of the clean ones — what tests/test_gpu_align_models.py then asks of the device."""
    fx = cases.fixture()
    h = cases.HS[0]
    statuses = []
    for q, n in enumerate(cases.SIZES):
        lo, hi = fx["offset"][q], fx["offset"][q + 1]
        assert hi - lo == n
        if n < so.SAMPLE:
            statuses.append(cases.TOO_FEW)
            continue
        pairs, thr = fx["pairs"][lo:hi], fx["thr"][q]
        _, models, _, _, _, _, best, err, mask = so.pass_outcome(pairs, cases.SEED + q * cases.STRIDE, cases.H_BEGIN, h, thr,
                                                                 fx["min_extra"][q], cases.RMS)
        statuses.append(cases.status_of(n, best))
        if best < 0:
            continue
        _, keep, info = so.refine(pairs, models[best], mask, err, thr, cases.RMS, cases.ROUNDS)
        clean = fx["clean"][q]
        assert not keep[~clean].any(), q
        share = np.count_nonzero(keep[clean]) / np.count_nonzero(clean)
        assert share >= 0.99, (q, share)
        truth = np.concatenate([fx["sims"][q][1].reshape(9), fx["sims"][q][2], [fx["sims"][q][0]]])
        assert so.model_gap(truth, so.model_svd(pairs[keep != 0, :3], pairs[keep != 0, 3:])[0], pairs) < 1e-3, q
    assert statuses[cases.NO_MODEL_PAIR] == cases.NO_MODEL
    assert [s for s, n in zip(statuses, cases.SIZES) if n < 3] == [cases.TOO_FEW] * 2
    assert all(s == cases.OK for s, n in zip(statuses, cases.SIZES) if n >= 40 and n != 513)
    # the thresholds differ between the pairs, and so do the similarities
    assert len(set(fx["thr"].tolist())) == len(cases.SIZES)


def test_oracle_filler_rules():
    assert [cases.status_of(n, -1) for n in (0, 2, 3, 40)] == [cases.TOO_FEW, cases.TOO_FEW, cases.NO_MODEL, cases.NO_MODEL]
    assert cases.status_of(3, 0) == cases.OK and cases.status_of(2, 0) == cases.TOO_FEW
    f = cases.pass_filler(5)
    assert np.all(f["flags"] == _native.FIT_DEGENERATE) and f["model"].shape == (5, 13) and f["S"].shape == (5, 8)
    assert so.select(f["cnt"], f["s1"], f["s2"], f["flags"], 0.0, cases.RMS) == (-1, np.inf)


def test_stream_case_is_registered():
    assert cases.stream_cases.CASES["align_models"].entries == ("sfm_align_models",)
    assert "sfm_align_models" in cases.stream_cases.covered_entries()
    assert not cases.stream_cases.CASES["align_models"].synchronising


def test_drop_in_path():
    import lib.multiview.alignment as drop_in

    for name in ("align_models", "merge_frames", "inconsistent_alignments", "ModelAlignments", "ModelFrames",
                 "estimate_similarity_with_ransac"):
        assert getattr(drop_in, name) is getattr(al, name)
