"""The dense stage without a GPU (csrc/sfm_plane_sweep.hip): the header, the binding and the op tuples agree; the
workspace size; every ValueError of the Python layer; the NumPy helpers; the definition (tests/plane_sweep_oracle.py) on
hand-computed cases and its accuracy on rendered planes."""
import ctypes as C

import numpy as np
import pytest

import plane_sweep_cases as cases   # registers the stream case of the two entry points (see that module)
import plane_sweep_oracle as po
import stream_cases
from structure_from_motion_amd import _native, ops, synthetic
from structure_from_motion_amd.stereo import depth_maps as dm


# ---- the layers agree -------------------------------------------------------------------------------------------------------------
def test_header_binding_and_ops_agree():
    import test_stream_cases_host as header

    functions = header.declared()
    for name in ("sfm_plane_sweep", "sfm_filter_depth_maps"):
        params, comment = functions[name]
        assert name in _native.SIGNATURES and params.endswith("void* stream")
        assert len(_native.SIGNATURES[name]) == params.count(",") + 1
        assert comment and header.SYNC_PHRASE not in comment
        assert name in stream_cases.covered_entries()
    assert "sfm_plane_sweep_workspace_bytes" in functions and "sfm_plane_sweep_workspace_bytes" in _native.OTHER_SYMBOLS
    with open(header.HEADER) as f:
        text = f.read()
    assert "#define SFM_SWEEP_OK 0" in text and "#define SFM_SWEEP_BAD_REFERENCE 1" in text
    assert _native.SWEEP_STATUS == ("ok", "bad_reference") and _native.ABI_VERSION == 15
    lib = _native.load()
    for name in ("sfm_plane_sweep", "sfm_filter_depth_maps", "sfm_plane_sweep_workspace_bytes"):
        assert hasattr(lib, name)


def test_the_depth_map_ops_are_listed_beside_the_pinned_tuples():
    assert ops.DEPTH_MAP_OPS == ("plane_sweep", "plane_sweep_", "filter_depth_maps", "filter_depth_maps_")
    others = (ops.FUNCTIONAL_OPS + ops.INPLACE_OPS + ops.LATER_FUNCTIONAL_OPS + ops.REGISTER_VIEWS_OPS + ops.SIMILARITY_OPS +
              ops.ALIGN_MODELS_OPS)
    assert not set(ops.DEPTH_MAP_OPS) & set(others)
    with open(ops.OPS_LIB_PATH.replace("libsfm_torch_ops.so", "sfm_torch_ops.cpp")) as f:
        source = f.read()
    for name in ops.DEPTH_MAP_OPS:
        assert f'm.def("{name}(' in source and source.count(f'm.impl("{name}",') == 2   # the device kernel and the Meta kernel


def test_the_stream_case_runs_both_entry_points():
    case = stream_cases.CASES["plane_sweep"]
    assert case.entries == ("sfm_plane_sweep", "sfm_filter_depth_maps") and case.ops == () and not case.synchronising


# ---- the workspace ------------------------------------------------------------------------------------------------------------------
def test_workspace_bytes_are_monotone_and_refused_sizes_give_minus_one():
    size = _native.load().sfm_plane_sweep_workspace_bytes
    base = (4, 48, 64, 4, 2, 9)
    assert size(*base) >= 4 * 2 * 9 * 72 and size(*base) % 256 == 0
    assert size(1, 4, 4, 0, 1, 1) >= 0   # no reference: a no-op with a workspace of any size
    for at, more in ((3, 5), (4, 3), (5, 10)):   # the homographies grow with refs, sources and depths alone
        bigger = list(base)
        bigger[at] = more
        assert size(*bigger) > size(*base)
    for at in (0, 1, 2):
        bigger = list(base)
        bigger[at] *= 2
        assert size(*bigger) == size(*base)
    assert size(4, 48, 64, 65535, 8, 4096) == ((65535 * 8 * 4096 * 72 + 255) // 256) * 256
    refused = [(0, 48, 64, 4, 2, 9), (2**31, 48, 64, 4, 2, 9), (4, 3, 64, 4, 2, 9), (4, 48, 3, 4, 2, 9), (4, 2**16, 2**15, 4, 2, 9),
               (4, 48, 64, -1, 2, 9), (4, 48, 64, 65536, 2, 9), (4, 48, 64, 4, 0, 9), (4, 48, 64, 4, 9, 9), (4, 48, 64, 4, 2, 0),
               (4, 48, 64, 4, 2, 4097), (4, -48, -64, 4, 2, 9)]
    for sizes in refused:
        assert size(*sizes) == -1, sizes


# ---- the Python layer refuses before any device work -------------------------------------------------------------------------------
def _good():
    sc = cases.scene(16, 20, views=3, seed=3)
    return dict(images=sc["images"], K=sc["K"], poses=sc["poses"], depths=np.array([4.0, 5.0, 6.0]))


@pytest.mark.parametrize("change", [
    dict(images=np.zeros((3, 16, 20), dtype=np.float32)), dict(images=np.zeros((16, 20), dtype=np.uint8)),
    dict(images=np.zeros((3, 7, 20), dtype=np.uint8)), dict(images=np.zeros((3, 16, 7), dtype=np.uint8)),
    dict(images=np.zeros((0, 16, 20), dtype=np.uint8)), dict(images=np.zeros((3, 11, 20), dtype=np.uint8), radius=5),
    dict(radius=0), dict(radius=6), dict(radius=2.0), dict(radius=True),
    dict(K=np.eye(4)), dict(K=np.array([[1.0, 0, 0], [0.5, 1, 0], [0, 0, 1]])), dict(K=np.array([[1.0, 0, 0], [0, 1, 0], [0, 0, 2]])),
    dict(K=np.array([[0.0, 0, 0], [0, 1, 0], [0, 0, 1]])), dict(K=np.array([[np.nan, 0, 0], [0, 1, 0], [0, 0, 1]])),
    dict(poses=np.zeros((2, 12))), dict(poses=np.zeros((3, 3, 4))), dict(poses=np.full((3, 12), np.inf)),
    dict(depths=np.zeros((2, 3))), dict(depths=np.zeros((3, 0))), dict(depths=np.zeros(4097)), dict(depths=np.zeros((3, 3, 1))),
    dict(refs=[0, 3]), dict(refs=[-1]), dict(refs=[[0, 1]]), dict(refs=[0.5]),
    dict(sources=[[1], [0]]), dict(sources=[[1, 2, 0, 1, 2, 0, 1, 2, 0]] * 3), dict(sources=np.zeros((3, 0), dtype=np.int32)),
    dict(sources=[[3], [0], [0]]), dict(sources=[[-2], [0], [0]]), dict(sources=[[0.5], [0.0], [0.0]]), dict(sources=[1, 0, 0]),
    dict(top_k=-1), dict(top_k=1.5), dict(min_sources=0), dict(min_sources="1"), dict(min_variance=-1.0), dict(min_variance=np.nan),
    dict(min_variance=np.inf), dict(max_refs_per_call=0),
])
def test_compute_depth_maps_refuses(change):
    with pytest.raises(ValueError):
        dm.compute_depth_maps(**{**_good(), **change})


def test_sources_default_needs_two_views():
    good = _good()
    with pytest.raises(ValueError):
        dm.compute_depth_maps(good["images"][:1], good["K"], good["poses"][:1], good["depths"])


@pytest.mark.parametrize("change", [
    dict(depth_maps=np.zeros((16, 20))), dict(depth_maps=np.zeros((0, 16, 20))), dict(depth_maps=np.zeros((3, 0, 20))),
    dict(K=np.eye(2)), dict(poses=np.zeros((4, 12))), dict(sources=[[1], [0]]), dict(sources=[[3], [0], [0]]),
    dict(max_pixel_error=-1.0), dict(max_pixel_error=np.nan), dict(max_relative_depth_error=-0.1), dict(max_relative_depth_error=np.inf),
    dict(min_consistent=-1), dict(min_consistent=1.0),
    dict(depth_maps=dm.DepthMaps(np.zeros((2, 16, 20)), np.zeros((2, 16, 20), np.int32), np.zeros((2, 16, 20)), np.array([1, 0]), None,
                                 np.zeros((2, 16, 20), np.uint8))),
])
def test_filter_depth_maps_refuses(change):
    good = _good()
    args = dict(depth_maps=np.full((3, 16, 20), 5.0), K=good["K"], poses=good["poses"], sources=[[1], [0], [1]])
    with pytest.raises(ValueError):
        dm.filter_depth_maps(**{**args, **change})


# ---- the helpers ---------------------------------------------------------------------------------------------------------------------
def test_depth_hypotheses_are_uniform_in_inverse_depth():
    z = dm.depth_hypotheses(2.0, 8.0, 7)
    assert z[0] == 2.0 and z[-1] == 8.0 and np.all(np.diff(z) > 0)
    steps = np.diff(1.0 / z)
    assert np.allclose(steps, (1 / 8.0 - 1 / 2.0) / 6, rtol=1e-12, atol=0)
    assert np.array_equal(dm.depth_hypotheses(3.0, 9.0, 1), [3.0]) and np.array_equal(dm.depth_hypotheses(3.0, 3.0, 2), [3.0, 3.0])
    for bad in ((0.0, 1.0, 3), (2.0, 1.0, 3), (1.0, np.inf, 3), (np.nan, 1.0, 3), (1.0, 2.0, 0), (1.0, 2.0, 4097), (1.0, 2.0, 2.5)):
        with pytest.raises(ValueError):
            dm.depth_hypotheses(*bad)


def test_select_source_views_ties_and_padding():
    # view 0 sees points 0-5; view 1 sees 0-3 (4 shared); views 2 and 3 see 4, 5 and 0, 1 (2 shared each: a tie); view 4 sees 9 alone
    cam = [0] * 6 + [1] * 4 + [2] * 2 + [3] * 2 + [4]
    pt = [0, 1, 2, 3, 4, 5, 0, 1, 2, 3, 4, 5, 0, 1, 9]
    got = dm.select_source_views(cam, pt, 5, 3)
    assert got.dtype == np.int32 and got.shape == (5, 3)
    assert got[0].tolist() == [1, 2, 3]        # 4 shared, then the tie of 2 to the lower index
    assert got[1].tolist() == [0, 3, -1]       # view 2 shares nothing with view 1
    assert got[2].tolist() == [0, -1, -1] and got[3].tolist() == [0, 1, -1] and got[4].tolist() == [-1, -1, -1]
    assert dm.select_source_views(cam, pt, 5, 1)[:, 0].tolist() == [1, 0, 0, 0, -1]
    assert dm.select_source_views([], [], 2, 2).tolist() == [[-1, -1], [-1, -1]]
    for bad in ((cam, pt[:-1], 5, 3), (cam, pt, 4, 3), (cam, pt, 5, 0), (cam, pt, 5, 9), ([0.5], [1.0], 2, 1)):
        with pytest.raises(ValueError):
            dm.select_source_views(*bad)


def test_depth_ranges_on_a_hand_made_model():
    poses = np.stack([cases.pose(), cases.pose(t=(0.0, 0.0, 1.0)), cases.pose()])   # view 1 sees everything one unit deeper
    points = np.array([[0.0, 0.0, 2.0], [1.0, 0.0, 4.0], [0.0, 1.0, -3.0], [0.0, 0.0, np.nan]])
    cam, pt = [0, 0, 0, 1, 1, 0], [0, 1, 2, 0, 1, 3]
    near, far = dm.depth_ranges(poses, points, cam, pt, margin=0.25)
    assert near[0] == 2.0 / 1.25 and far[0] == 4.0 * 1.25       # the point behind the camera and the NaN are left out
    assert near[1] == 3.0 / 1.25 and far[1] == 5.0 * 1.25
    assert np.isnan(near[2]) and np.isnan(far[2])               # a view without observations
    for bad in (dict(poses=np.zeros((3, 11))), dict(points=np.zeros((4, 2))), dict(margin=-0.1), dict(cam=[0, 5]), dict(pt=[0, 4])):
        args = dict(poses=poses, points=points, cam=[0, 1], pt=[0, 1], margin=0.1)
        args.update(bad)
        with pytest.raises(ValueError):
            dm.depth_ranges(args["poses"], args["points"], args["cam"], args["pt"], args["margin"])


def test_plane_views_renders_exact_depths_and_occlusions():
    sc = cases.scene(48, 64, views=5, seed=2, two_planes=True)
    assert sc["images"].dtype == np.uint8 and sc["images"].shape == (5, 48, 64) and sc["images"].std() > 30
    front = sc["plane"] == 1
    assert front.any() and np.allclose(sc["depth"][2][front[2]], 3.6)          # the middle camera looks along Z
    ramp = cases.scene(48, 64, views=5, seed=1)["depth"][2]
    assert np.all(np.diff(ramp, axis=1) > 0)                                       # a slanted plane: a depth ramp
    flat = synthetic.plane_views(8, 8, [cases.pose()], [((0, 0, 2.0), (1, 0, 0), (0, 1, 0), (0.01, 0.01))], seed=0, K=cases.exact_camera())
    assert flat["plane"][0, 4, 16 - 16] == -1 and np.isnan(flat["depth"][0, 0, 0])   # rays that miss the bounded plane


# ---- the definition on hand-computed cases -----------------------------------------------------------------------------------------
def _textured(height, width, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(height, width)).astype(np.uint8)


def test_oracle_identity_pose_costs_exactly_zero():
    image = _textured(12, 14, 0)
    image[:, :5] = 77   # a flat region: its windows fail the variance gate
    out = po.plane_sweep(np.stack([image, image]), cases.exact_camera(), np.stack([cases.pose(), cases.pose()]), [0], [[1]], [[3.0]], 1)
    assert np.array_equal(po.homography(cases.exact_camera(), cases.pose(), cases.pose(), 3.0), np.eye(3))
    cost, index = out["cost"][0], out["index"][0]
    valid = np.zeros((12, 14), dtype=bool)
    # windows that hold a textured column (x >= 4) and touch neither the last column nor the last row, where u < W - 1 or
    # v < H - 1 fails and the sample is invalid
    valid[1:10, 4:12] = True
    assert np.array_equal(index >= 0, valid)
    assert np.all(cost[valid] == 0.0) and np.all(np.isnan(cost[~valid])) and np.all(out["depth"][0][valid] == 3.0)
    assert po.same_bytes(out["volume"][0, 0], cost)


def test_oracle_finds_a_pure_one_pixel_shift():
    ref = _textured(12, 20, 1)
    src = np.zeros_like(ref)
    src[:, 1:] = ref[:, :-1]   # the source shows the reference one pixel to the right
    poses = np.stack([cases.pose(), cases.pose(t=(1.0 / 16.0, 0.0, 0.0))])   # 64 / 16 / z pixels: one pixel at z = 4
    G = po.homography(cases.exact_camera(), poses[0], poses[1], 4.0)
    assert np.array_equal(G, [[1.0, 0.0, 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    out = po.plane_sweep(np.stack([ref, src]), cases.exact_camera(), poses, [0], [[1]], [[2.0, 4.0, 8.0]], 2)
    inner = (slice(2, 9), slice(2, 16))   # windows that touch neither the last row (v < H - 1) nor a sample beyond x + 1 < W - 1
    assert np.all(out["index"][0][inner] == 1) and np.all(out["cost"][0][inner] == 0.0)
    assert np.all(out["volume"][0, 0][2:9, 2:15] > 0.0) and np.all(out["volume"][0, 2][inner] > 0.0)   # (two pixels at z = 2)
    # the parabola step moves the depth off the hypothesis, towards the neighbour of lower cost, by less than half a step
    depth = out["depth"][0][2:9, 2:15]
    assert np.all((depth > 1.0 / (0.5 * (1 / 4.0 + 1 / 2.0))) & (depth < 1.0 / (0.5 * (1 / 4.0 + 1 / 8.0))))
    assert np.all(out["index"][0][:, 18:] == -1)   # x + 1 >= W - 1: the sample leaves the source


def test_oracle_constant_image_has_no_valid_score():
    images = np.full((2, 10, 10), 128, dtype=np.uint8)
    poses = np.stack([cases.pose(), cases.pose(t=(0.1, 0.0, 0.0))])
    out = po.plane_sweep(images, cases.exact_camera(), poses, [0], [[1]], [[2.0, 4.0]], 1)
    assert np.all(out["index"] == -1) and np.all(np.isnan(out["volume"])) and np.all(np.isnan(out["depth"])) and out["status"][0] == 0
    free = po.plane_sweep(images, cases.exact_camera(), poses, [0], [[1]], [[2.0, 4.0]], 1, min_variance=0.0)
    assert np.all(free["index"] == -1)   # 0 / 0: the score is not finite


def test_oracle_aggregation_sources_and_bad_references():
    sc = cases.scene(20, 24, views=4, seed=5)
    z = cases.hypotheses(sc, 3)
    args = (sc["images"], sc["K"], sc["poses"])
    one = po.plane_sweep(*args, [1], [[0]], [z], 2)["volume"][0]
    two = po.plane_sweep(*args, [1], [[2]], [z], 2)["volume"][0]
    both = po.plane_sweep(*args, [1], [[0, 2, 1, -1]], [z], 2)["volume"][0]   # the reference itself and -1 are absent
    with np.errstate(all="ignore"):
        lo, hi = np.fmin(one, two), np.fmax(one, two)
        mean = np.where(np.isfinite(one) & np.isfinite(two), (lo + hi) / 2.0, lo)
    assert po.same_bytes(both, mean)
    assert po.same_bytes(po.plane_sweep(*args, [1], [[0, 2]], [z], 2, top_k=1)["volume"][0], lo)
    need_two = po.plane_sweep(*args, [1], [[0, 2]], [z], 2, min_sources=2)["volume"][0]
    assert np.array_equal(np.isfinite(need_two), np.isfinite(one) & np.isfinite(two))
    bad = po.plane_sweep(*args, [4, 1, -1], [[0, 2]] * 3, [z] * 3, 2)
    assert bad["status"].tolist() == [1, 0, 1] and np.all(bad["index"][[0, 2]] == -1) and np.all(np.isnan(bad["volume"][[0, 2]]))
    invalid = po.plane_sweep(*args, [1], [[0, 2]], [[z[0], -z[1], np.nan]], 2)
    assert np.all(np.isnan(invalid["volume"][0, 1:])) and np.all(invalid["index"][0] <= 0)


def test_oracle_filter_on_the_exact_boundary():
    case = cases.filter_boundary_case()
    args = (case["depth"], case["K"], case["poses"], case["refs"], case["sources"])
    out = po.filter_depth_maps(*args, max_pixel_error=8.0, max_relative_depth_error=0.5, min_consistent=1)
    count = out["count"][0]
    assert count[case["on_boundary"]] == 1 and count[case["beyond"]] == 0 and count[case["hole"]] == 0
    assert out["filtered"][0][case["on_boundary"]] == 4.0 and np.isnan(out["filtered"][0][case["beyond"]])
    y, x = case["on_boundary"]
    assert np.array_equal(out["points"][0, y, x], [(x - 16.0) / 64.0 * 4.0, (y - 4.0) / 64.0 * 4.0, 4.0])
    assert np.all(np.isnan(out["points"][0][count == 0])) and np.all(count[:, 24:] == 0)   # no depth, no count
    tighter = po.filter_depth_maps(*args, max_pixel_error=np.nextafter(8.0, 0.0), max_relative_depth_error=0.5, min_consistent=1)
    assert tighter["count"][0][case["on_boundary"]] == 0
    nearer = po.filter_depth_maps(*args, max_pixel_error=8.0, max_relative_depth_error=np.nextafter(0.5, 0.0), min_consistent=1)
    assert nearer["count"][0][case["on_boundary"]] == 0
    assert np.all(po.filter_depth_maps(*args, 8.0, 0.5, 0)["filtered"][0][:, :24] == 4.0)   # min_consistent 0 keeps every depth


# ---- the accuracy of the definition ------------------------------------------------------------------------------------------------
def test_oracle_accuracy_on_a_slanted_plane():
    out, truth, _ = cases.slanted_accuracy()
    keep = np.ones(out["index"].shape, dtype=bool)
    assert cases.interior(out["index"].shape, 3).sum() == cases.SLANTED_INTERIOR
    right, _ = cases.within_one(out["index"], truth, keep, 3)
    assert right >= cases.SLANTED_WITHIN_ONE
    assert right >= 0.94 * cases.SLANTED_INTERIOR   # what makes the count worth asserting


def test_oracle_accuracy_after_the_filter_on_two_planes():
    sweep, kept, truth = cases.two_plane_accuracy()
    keep = np.ones(sweep["index"].shape, dtype=bool)
    right_before, wrong_before = cases.within_one(sweep["index"], truth, keep, 3)
    right_after, wrong_after = cases.within_one(sweep["index"], truth, np.isfinite(kept["filtered"]), 3)
    assert right_before >= cases.TWO_PLANE_RIGHT_BEFORE and wrong_before <= cases.TWO_PLANE_WRONG_BEFORE
    assert right_after >= cases.TWO_PLANE_RIGHT_AFTER and wrong_after <= cases.TWO_PLANE_WRONG_AFTER
    # the filter is worth having: it removes two thirds of the wrong depths and keeps five sixths of the right ones
    assert wrong_after * 3 <= wrong_before and right_after * 6 >= right_before * 5
    cloud = dm.point_cloud(dm.FilteredDepthMaps(kept["filtered"], kept["count"], kept["points"], np.arange(5),
                                                cases.scene(48, 64, views=5, seed=2, two_planes=True)["images"]))
    assert len(cloud[0]) == np.isfinite(kept["filtered"]).sum() == len(cloud[1]) == len(cloud[2]) and cloud[1].dtype == np.uint8
    assert np.array_equal(np.bincount(cloud[2], minlength=5), np.isfinite(kept["filtered"]).sum(axis=(1, 2)))
