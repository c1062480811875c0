"""Tracks from pairwise matches on the MI355X (csrc/sfm_track_build.hip): exact parity with the plain-Python oracle of
tests/track_build_oracle.py on every output, recovery of a scene's true tracks, adversarial graphs under a time budget
(a long chain, a contended star, one huge conflict component), empty inputs, the bad-index record, order independence and
repeatability, the op layer, the public API, triangulation of the built tracks and the N-view app on built tracks."""
import time

import numpy as np
import pytest
import torch

import track_build_oracle as tbo
from structure_from_motion_amd import synthetic

pytestmark = pytest.mark.gpu

OUTPUTS = ("component", "track", "status", "camera_index", "point_index", "feature_index")


@pytest.fixture(scope="module")
def dev(native_lib):
    from structure_from_motion_amd import device

    return device.require_gpu()


def _device_call(dev, off, pairs, mo, mi, F=None):
    from structure_from_motion_amd import device

    t = lambda a, shape: torch.as_tensor(np.asarray(a, dtype=np.int32).reshape(shape), device=dev)
    F = int(off[-1]) if F is None else F
    out = device.build_tracks(t(off, (-1,)), t(pairs, (-1, 2)), t(mo, (-1,)), t(mi, (-1, 2)), F)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in zip(OUTPUTS, out[:6])}
    res["info"] = device.read_track_build_info(out[6])
    assert res["info"].status != 2, "a bounded device loop gave up"
    return res


def _assert_parity(got, want):
    for k in OUTPUTS:
        assert np.array_equal(got[k].astype(np.int64), want[k].astype(np.int64)), k
    i = got["info"]
    assert (i.status, i.components, i.tracks, i.observations, i.conflicts, i.unmatched) == want["info"]


def _graph(images, features, neighbours, per_pair, wrong, seed):
    g = synthetic.match_graph(images, features, neighbours, per_pair, wrong_fraction=wrong, seed=seed)
    return g["image_offset"], g["pairs"], g["match_offset"], g["match_index"]


@pytest.mark.parametrize("images,features,neighbours,per_pair,wrong,seed", [
    (8, 50, 2, 20, 0.0, 0), (8, 50, 2, 20, 0.2, 1), (30, 300, 4, 100, 0.05, 2), (64, 1000, 5, 300, 0.0, 3),
    (64, 1000, 5, 300, 0.1, 4), (200, 5000, 3, 2000, 0.02, 5)])
def test_parity_with_oracle(dev, images, features, neighbours, per_pair, wrong, seed):
    args = _graph(images, features, neighbours, per_pair, wrong, seed)
    _assert_parity(_device_call(dev, *args), tbo.build_tracks(*args))


def test_parity_with_oracle_at_a_million_features(dev):
    """10^6 features, 3 * 10^6 matches, 1 % wrong (the oracle takes a few seconds here)."""
    args = _graph(250, 4000, 6, 2000, 0.01, 7)
    assert int(args[0][-1]) == 10**6 and len(args[3]) == 3 * 10**6
    _assert_parity(_device_call(dev, *args), tbo.build_tracks(*args))


@pytest.mark.parametrize("seed", range(4))
def test_parity_on_random_small_graphs(dev, seed):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 40, 12)
    ps, ms = [], []
    for _ in range(40):
        a, b = rng.choice(12, 2, replace=False)
        k = int(rng.integers(0, 10)) if counts[a] and counts[b] else 0
        ps.append((a, b))
        ms.append(np.column_stack([rng.integers(0, max(counts[a], 1), k), rng.integers(0, max(counts[b], 1), k)]))
    args = tbo.from_lists(counts, ps, ms)
    _assert_parity(_device_call(dev, *args), tbo.build_tracks(*args))


def test_recovers_the_scene_tracks(dev):
    """Clean matches (no wrong matches, no scene outliers, no verification) give exactly the scene's tracks."""
    from structure_from_motion_amd.multiview.tracks import build_tracks

    scene = synthetic.multi_view_scene(8, 1500, seed=3, outlier_fraction=0.0)
    pm = synthetic.pairwise_matches(scene, window=7, wrong_fraction=0.0, seed=5)
    r = build_tracks(pm["features"], pm["pairs"], pm["matches"])
    truth = np.concatenate(pm["feature_points"])
    assert r.info.conflicts == 0 and r.info.unmatched == 0 and r.info.status == 0
    assert r.info.tracks == len(np.unique(scene["point_indices"])) and r.info.observations == len(truth)
    true_pt = truth[r.feature_indices]
    # the same partition: each track is one true point and each true point one track
    assert np.all(true_pt[1:][r.point_indices[1:] == r.point_indices[:-1]] ==
                  true_pt[:-1][r.point_indices[1:] == r.point_indices[:-1]])
    assert len(np.unique(true_pt)) == r.info.tracks
    # tracks numbered by their first (smallest) feature
    first = r.feature_indices[np.r_[True, r.point_indices[1:] != r.point_indices[:-1]]]
    assert np.all(np.diff(first) > 0)
    assert np.array_equal(r.component[first], first)


def _timed(dev, args, budget_s):
    t0 = time.perf_counter()
    got = _device_call(dev, *args)
    elapsed = time.perf_counter() - t0
    print(f"{int(args[0][-1])} features, {len(args[3])} matches: {elapsed:.3f} s")
    assert elapsed < budget_s
    return got


def test_long_chain_listed_from_the_far_end(dev):
    n = 10**5
    off = np.arange(n + 1)
    pairs = np.array([(i, i + 1) for i in range(n - 2, -1, -1)])
    mo = np.arange(n)
    mi = np.zeros((n - 1, 2), dtype=np.int64)
    _device_call(dev, off, pairs, mo, mi)   # warm-up
    got = _timed(dev, (off, pairs, mo, mi), 5.0)
    assert np.all(got["component"] == 0) and np.all(got["status"] == tbo.OK)
    assert np.array_equal(got["feature_index"], np.arange(n)) and np.all(got["point_index"] == 0)


def test_star_with_the_largest_centre(dev):
    n = 10**5   # leaves in images 0 .. n-1, centre in image n: every hook contends on the leaves' roots
    off = np.arange(n + 2)
    pairs = np.column_stack([np.full(n, n), np.arange(n)])
    mo = np.arange(n + 1)
    mi = np.zeros((n, 2), dtype=np.int64)
    got = _timed(dev, (off, pairs, mo, mi), 5.0)
    assert np.all(got["component"] == 0) and got["info"].tracks == 1 and got["info"].observations == n + 1
    _assert_parity(got, tbo.build_tracks(off, pairs, mo, mi))


def test_one_huge_conflict_component(dev):
    """2.5 * 10^5 features in 10 images chained into one component: the long-run grouping path."""
    per, I = 25000, 10
    off = np.arange(I + 1) * per
    pairs, ms = [], []
    for i in range(I - 1):
        pairs.append((i, i + 1))
        ms.append(np.column_stack([np.arange(per), np.arange(per)]))
        pairs.append((i + 1, i))   # a shifted link back: two features of one image in one component
        ms.append(np.column_stack([np.arange(per), (np.arange(per) + 1) % per]))
    args = tbo.from_lists(np.full(I, per), pairs, ms)
    got = _timed(dev, args, 5.0)
    assert got["info"].conflicts == 1 and got["info"].tracks == 0 and np.all(got["status"] == tbo.CONFLICT)
    _assert_parity(got, tbo.build_tracks(*args))


def test_duplicate_and_reversed_pairs(dev):
    counts = [5, 4, 6]
    base = [(0, 1), (1, 2)]
    bm = [np.array([[0, 0], [1, 1], [4, 3]]), np.array([[0, 5], [2, 2]])]
    dup = base + [(1, 0), (0, 1)] + [(2, 1)]
    dm = bm + [bm[0][:, ::-1], bm[0][[2, 0]]] + [bm[1][:, ::-1]]
    a = _device_call(dev, *tbo.from_lists(counts, base, bm))
    b = _device_call(dev, *tbo.from_lists(counts, dup, dm))
    for k in OUTPUTS:
        assert np.array_equal(a[k], b[k]), k
    _assert_parity(b, tbo.build_tracks(*tbo.from_lists(counts, dup, dm)))


def test_empty_inputs(dev):
    got = _device_call(dev, [0], np.zeros((0, 2)), [0], np.zeros((0, 2)))
    assert got["info"].status == 0 and got["info"].tracks == 0 and len(got["component"]) == 0
    args = tbo.from_lists([0, 3, 0, 2], [(0, 1), (1, 3), (2, 0)], [np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 2))])
    got = _device_call(dev, *args)
    assert got["info"].unmatched == 5 and np.all(got["status"] == tbo.UNMATCHED)
    _assert_parity(got, tbo.build_tracks(*args))
    args = tbo.from_lists([0, 0], [(0, 1)], [np.zeros((0, 2))])
    _assert_parity(_device_call(dev, *args), tbo.build_tracks(*args))


@pytest.mark.parametrize("case", ["local", "image", "same_image", "offsets", "match_offsets"])
def test_bad_index_record(dev, case):
    off, pairs, mo, mi = [np.array(a) for a in tbo.from_lists([3, 2, 4], [(0, 1), (1, 2)], [[(0, 0), (2, 1)], [(1, 3)]])]
    if case == "local":
        mi[2, 1] = 4
    elif case == "image":
        pairs[1, 1] = 3
    elif case == "same_image":
        pairs[0, 1] = 0
    elif case == "offsets":
        off[1], off[2] = 4, 3
    else:
        mo[1] = 3
    got = _device_call(dev, off, pairs, mo, mi, F=9)
    assert got["info"].status == 1 and got["info"].tracks == 0 and got["info"].observations == 0
    assert np.all(got["status"] == tbo.BAD_INDEX) and np.all(got["track"] == -1) and np.all(got["camera_index"] == -1)


def test_order_independence_and_repeatability(dev):
    rng = np.random.default_rng(11)
    g = synthetic.match_graph(40, 600, 4, 200, wrong_fraction=0.1, seed=11)
    Q = len(g["pairs"])
    per = [g["match_index"][g["match_offset"][q]:g["match_offset"][q + 1]] for q in range(Q)]
    counts = np.diff(g["image_offset"])
    ref = _device_call(dev, *tbo.from_lists(counts, g["pairs"], per))
    for trial in range(3):
        order = rng.permutation(Q)
        flip = rng.random(Q) < 0.5
        ps = [tuple(g["pairs"][q][::-1]) if f else tuple(g["pairs"][q]) for q, f in zip(order, flip[order])]
        ms = [per[q][rng.permutation(len(per[q]))][:, ::-1 if f else 1] for q, f in zip(order, flip[order])]
        got = _device_call(dev, *tbo.from_lists(counts, ps, ms))
        for k in OUTPUTS:
            assert np.array_equal(got[k], ref[k]), (trial, k)
    again = _device_call(dev, *tbo.from_lists(counts, g["pairs"], per))
    for k in OUTPUTS:
        assert np.array_equal(again[k], ref[k]), k


def test_inplace_op_and_opcheck(dev):
    from structure_from_motion_amd import device, ops

    op = ops.load()
    args = [torch.as_tensor(a, dtype=torch.int32, device=dev) for a in _graph(12, 200, 3, 60, 0.1, 9)]
    F = 12 * 200
    fun = device.build_tracks(*args, F)
    out = tuple(torch.full_like(t, 7) for t in fun)
    device.build_tracks(*args, F, out=out)
    for a, b in zip(fun, out):
        assert torch.equal(a, b)
    torch.library.opcheck(op.build_tracks.default, (*args, F))
    torch.library.opcheck(op.build_tracks_.default, (*args, F, *[torch.empty_like(t) for t in fun]))


def test_public_api_equals_device_call(dev):
    from structure_from_motion_amd.multiview.tracks import build_tracks
    from structure_from_motion_amd.feature_matching.matching import Match
    from structure_from_motion_amd.common.feature import Feature

    scene = synthetic.multi_view_scene(5, 400, seed=2)
    pm = synthetic.pairwise_matches(scene, window=2, wrong_fraction=0.1, seed=3)
    r = build_tracks(pm["features"], pm["pairs"], pm["matches"])
    args = tbo.from_lists([len(f) for f in pm["features"]], pm["pairs"], pm["matches"])
    d = _device_call(dev, *args)
    M = r.info.observations
    assert np.array_equal(r.camera_indices, d["camera_index"][:M]) and np.array_equal(r.point_indices, d["point_index"][:M])
    assert np.array_equal(r.feature_indices, d["feature_index"][:M]) and np.array_equal(r.component, d["component"])
    assert np.array_equal(r.track_of_feature, d["track"]) and np.array_equal(r.feature_status, d["status"])
    assert np.array_equal(r.pixels, np.concatenate(pm["features"])[r.feature_indices])
    # Feature / Match lists give the same result
    feats = [[Feature(float(x), float(y)) for x, y in f] for f in pm["features"]]
    matches = [[Match(a_index=int(a), b_index=int(b)) for a, b in m] for m in pm["matches"]]
    r2 = build_tracks(feats, pm["pairs"], matches)
    assert np.array_equal(r2.feature_indices, r.feature_indices) and np.array_equal(r2.pixels, r.pixels)


def test_built_tracks_triangulate_the_scene(dev):
    from structure_from_motion_amd import device
    from structure_from_motion_amd.multiview.tracks import build_tracks, triangulate_tracks

    scene = synthetic.multi_view_scene(6, 500, seed=8, noise_px=0.0, outlier_fraction=0.0)
    pm = synthetic.pairwise_matches(scene, window=5, wrong_fraction=0.0, seed=9)
    r = build_tracks(pm["features"], pm["pairs"], pm["matches"])
    t = triangulate_tracks(scene["K"], scene["poses_true"], r.camera_indices, r.point_indices, r.pixels)
    assert np.all(t.status == device.TRACKS_OK)
    truth = np.concatenate(pm["feature_points"])[r.feature_indices]
    first = np.r_[True, r.point_indices[1:] != r.point_indices[:-1]]
    assert np.max(np.abs(t.points - scene["points_true"][truth[first]])) < 1e-9


def test_multi_view_app_on_built_tracks(dev):
    """Registration from tracks built out of RANSAC-verified matches.  The margins are predictions checked against the
    measured run (see profiles/track_build/README.md), in the style of the five-point app test."""
    from apps import sfm_multi_view

    given = sfm_multi_view.run()
    built = sfm_multi_view.run(tracks="matches")
    print("given:", {k: given[k] for k in ("views_registered", "rms_px", "points_ok")},
          max(given["rotation_error_rad"].values()), max(given["translation_error"].values()))
    print("matches:", {k: built[k] for k in ("views_registered", "rms_px", "points_ok", "track_build")},
          max(built["rotation_error_rad"].values()), max(built["translation_error"].values()))
    assert built["views_registered"] == 8 == given["views_registered"]
    assert max(built["rotation_error_rad"].values()) <= max(given["rotation_error_rad"].values()) + 2e-3
    assert max(built["translation_error"].values()) <= max(given["translation_error"].values()) + 2e-2
    assert built["track_build"]["pure_track_fraction"] >= 0.9
