"""The dense stage on the GPU on a general camera and general poses, and as one chain from images to a mesh, against the chain of
the NumPy definitions (tests/dense_chain_cases.py; tests/test_dense_chain_host.py shows what that reference is worth), byte for
byte, a NaN equal to any NaN: each kernel alone, the chain with every stage fed by the device's own output, ``fuse_depth_maps``
without bounds, the three apps of the stage against what the definition gives on their own scenes, a mesh extraction beyond
1024 scan tiles and the widest depth groups of the semi-global smoothing."""
import functools

import numpy as np
import pytest

import dense_chain_cases as cases
import plane_sweep_cases as sweep_cases
import plane_sweep_oracle as po
import sgm_cases
import test_gpu_depth_fusion as fusion_tests
import test_gpu_plane_sweep as sweep_tests
import test_gpu_sgm as sgm_tests
import tsdf_cases
import tsdf_oracle as to

pytestmark = pytest.mark.gpu

MAP_NAMES = ("depth", "index", "cost")
FILTER = sweep_cases.TWO_PLANE_FILTER
FILTER_ARGS = (FILTER["max_pixel_error"], FILTER["max_relative_depth_error"], FILTER["min_consistent"])


def _libs():
    from structure_from_motion_amd.stereo import depth_maps as dm
    from structure_from_motion_amd.stereo import fusion

    return dm, fusion


def assert_maps(maps, want, names, what):
    sweep_tests.assert_same({name: getattr(maps, name) for name in names}, want, names, what)


def assert_kept(kept, want, what):
    sweep_tests.assert_same(dict(count=kept.count, filtered=kept.depth, points=kept.points), want, ("count", "filtered", "points"), what)


def assert_mesh(mesh, want, what):
    assert len(mesh.vertices) == want[2] > 0, f"{what}: {len(mesh.vertices)} triangles, the definition has {want[2]}"
    assert to.same_bytes(mesh.vertices, want[0]), f"{what}: the vertices differ from the definition"
    assert to.same_bytes(mesh.grey, want[1]), f"{what}: the grey values differ from the definition"


def device_maps(sc, smoothness, **kw):
    dm, _ = _libs()
    return dm.compute_depth_maps(sc["images"], sc["K"], sc["poses"], sc["depths"], sources=sc["sources"], radius=cases.RADIUS,
                                 top_k=cases.TOP_K, smoothness=smoothness, **kw)


# ---- each kernel alone on the general scene -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smoothness", [None, cases.SMOOTHNESS])
@pytest.mark.parametrize("per_call", [2, 64])
def test_depth_maps_on_the_general_scene(per_call, smoothness):
    sc = cases.scene(True)
    want = cases.chain(sc, smoothness)
    maps = device_maps(sc, smoothness, return_volume=True, max_refs_per_call=per_call)
    assert_maps(maps, {**want["maps"], "volume": want["sweep"]["volume"]}, MAP_NAMES + ("volume",), f"{per_call} references a call, {smoothness}")
    assert (want["maps"]["index"] >= 0).mean() > 0.7


@pytest.mark.parametrize("min_consistent", [1, 2])
def test_filter_on_the_general_scene(min_consistent):
    dm, _ = _libs()
    sc = cases.scene(True)
    maps = device_maps(sc, None)
    kept = dm.filter_depth_maps(maps, sc["K"], sc["poses"], sc["sources"], FILTER_ARGS[0], FILTER_ARGS[1], min_consistent)
    want = po.filter_depth_maps(maps.depth, sc["K"], sc["poses"], sc["refs"], sc["sources"], FILTER_ARGS[0], FILTER_ARGS[1], min_consistent)
    assert_kept(kept, want, f"min_consistent {min_consistent}")
    assert set(np.unique(want["count"])) == {0, 1, 2, 3, 4} and 0.5 < np.isfinite(want["filtered"]).mean() < 0.95


@functools.lru_cache(maxsize=None)
def ragged_volume():
    """17 x 9 x 4 voxels about the centre of the box of the kept points of the general scene, in its gauge, as large as the box
    allows: -> (dims, origin, voxel, truncation)."""
    sc = cases.scene(True)
    points = cases.chain(sc)["kept"]["points"]
    points = points[np.all(np.isfinite(points), axis=-1)]
    low, high = points.min(axis=0), points.max(axis=0)
    dims = (17, 9, 4)
    voxel = float(np.min((high - low) / np.array(dims)))
    origin = tuple(float(c) for c in 0.5 * (low + high) - 0.5 * voxel * np.array(dims))
    return dims, origin, voxel, 1.5 * voxel


@pytest.mark.parametrize("splits", [None, [(0, 2), (2, 5)]])
@pytest.mark.parametrize("with_grey", [True, False])
def test_integrate_on_the_general_scene(with_grey, splits):
    sc = cases.scene(True)
    dims, origin, voxel, truncation = ragged_volume()
    depth = cases.chain(sc)["kept"]["filtered"]
    inputs = dict(depth=depth, images=sc["images"], K=np.ascontiguousarray(sc["K"].reshape(9)), poses=sc["poses"])
    state = tsdf_cases.empty_state(dims, with_grey)
    got = fusion_tests.run_integrate(state, inputs, sc["refs"], origin, voxel, truncation, with_grey, splits)
    want = to.integrate(state, depth, sc["images"] if with_grey else None, sc["K"], sc["poses"], sc["refs"], origin, voxel, truncation)
    fusion_tests.assert_state(got, want, f"grey {with_grey} splits {splits}")
    assert want[1].max() == 5 and want[1].min() == 0 and (want[0] != 0.0).sum() > 200   # voxels that every view sees, and that none does


def test_a_small_sweep_through_the_entry_point_on_the_general_scene():
    sc = cases.small_scene()
    assert sc["images"].shape == (4, 37, 45) and sc["depths"].shape == (4, 5) and sc["sources"].shape == (4, 3)
    inp = dict(images=sc["images"], K=np.ascontiguousarray(sc["K"].reshape(9)), poses=sc["poses"], refs=sc["refs"], sources=sc["sources"],
               depths=sc["depths"])
    got, want = sweep_tests.check_sweep(inp, 2, top_k=2, min_sources=2)
    assert (want["index"] >= 0).mean() > 0.5 and set(np.unique(want["index"])) == {-1, 0, 1, 2, 3, 4}


# ---- the chain ------------------------------------------------------------------------------------------------------------------------
# on the general scene, and on the general camera and gauge with the cameras of the arc (untilted)
@pytest.mark.parametrize("tilt", [True, False])
@pytest.mark.parametrize("smoothness", [None, cases.SMOOTHNESS])
def test_the_chain_on_the_device_is_the_chain_of_the_definitions(smoothness, tilt):
    dm, fusion = _libs()
    sc = cases.scene(True, tilt=tilt)
    want = cases.chain(sc, smoothness)
    maps = device_maps(sc, smoothness)
    assert_maps(maps, want["maps"], MAP_NAMES, "depth maps")
    kept = dm.filter_depth_maps(maps, sc["K"], sc["poses"], sc["sources"], *FILTER_ARGS)
    assert_kept(kept, want["kept"], "filter")
    voxel = fusion.suggest_voxel_size(kept, sc["K"], cases.PIXELS)
    truncation = cases.TRUNCATION_VOXELS * voxel
    low, high = fusion.volume_bounds(kept, truncation)
    dims = np.maximum(np.ceil((high - low) / voxel).astype(np.int64), 2)
    assert voxel == want["voxel"] and np.array_equal(low, want["origin"]) and np.array_equal(dims, want["dims"])
    volume = fusion.TsdfVolume(low, voxel, dims, truncation, with_grey=True)
    volume.integrate(kept.depth, sc["K"], sc["poses"], images=sc["images"])
    fusion_tests.assert_state(volume.to_host(), want["fused"][:3], "TsdfVolume")
    assert_mesh(volume.extract_mesh(cases.MIN_COUNT), want["mesh"], "extract_mesh")
    # fuse_depth_maps lays the same volume itself
    assert_mesh(fusion.fuse_depth_maps(kept, sc["K"], sc["poses"], voxel, min_count=cases.MIN_COUNT, bounds=None), want["mesh"], "fuse_depth_maps")
    assert want["mesh"][2] > 3000


# ---- the apps -------------------------------------------------------------------------------------------------------------------------
def depth_map_figures(sc, result, truth):
    """What apps/depth_maps.py reports, from the definition's outputs ``result`` (a chain) on ``sc``."""
    dm, _ = _libs()
    index, depth, kept, z = result["maps"]["index"], result["maps"]["depth"], result["kept"], sc["depths"]
    V, H, W = index.shape
    inner = sweep_cases.interior((H, W), cases.RADIUS)
    cloud = dm.point_cloud(cases.filtered_maps(kept["filtered"], kept["points"], sc, kept["count"]))
    rows = []
    for v in range(V):
        with np.errstate(all="ignore"):
            nearest = np.abs(1.0 / truth[v][..., None] - 1.0 / z[v]).argmin(axis=-1)
            error = np.abs(depth[v] - truth[v]) / truth[v]
        right = (index[v] >= 0) & np.isfinite(truth[v]) & (np.abs(index[v] - nearest) <= 1)
        stays = np.isfinite(kept["filtered"][v]) & inner
        median = lambda values: float(np.median(values)) if len(values) else None   # noqa: E731
        rows.append({"view": v, "within_one_before": float((right & inner).sum() / inner.sum()),
                     "within_one_after": float((right & stays).sum() / max(int(stays.sum()), 1)), "kept": float(stays.sum() / inner.sum()),
                     "median_relative_error_before": median(error[inner & np.isfinite(error)]),
                     "median_relative_error_after": median(error[stays & np.isfinite(error)]), "cloud_points": int(np.sum(cloud[2] == v))})
    return {"per_view": rows, "cloud_points": int(len(cloud[0])), "mean_grey": float(cloud[1].mean())}


def surface_figures(sc, result, scene_poses, scale=1.0):
    """What apps/fuse_depth_maps.py reports, from the definition's outputs ``result`` (a chain) on ``sc``; the mesh goes into the
    scene's gauge as the app takes it there, through the first camera."""
    from apps.fuse_depth_maps import distance_to_planes

    _, fusion = _libs()
    vertices = result["mesh"][0]
    points, faces, _ = fusion.Mesh(vertices).weld()
    count = result["fused"][1] >= cases.MIN_COUNT
    cells = (count[:-1, :-1, :-1] & count[:-1, :-1, 1:] & count[:-1, 1:, :-1] & count[:-1, 1:, 1:] &
             count[1:, :-1, :-1] & count[1:, :-1, 1:] & count[1:, 1:, :-1] & count[1:, 1:, 1:])
    first, first_true = sc["poses"][0], scene_poses[0]

    def to_scene(X):
        camera = (X @ first[:9].reshape(3, 3).T + first[9:]) / scale
        return (camera - first_true[9:]) @ first_true[:9].reshape(3, 3)

    distance = distance_to_planes(to_scene(points)) / (result["voxel"] / scale)
    middle = scene_poses[len(scene_poses) // 2]
    centre = -middle[:9].reshape(3, 3).T @ middle[9:]
    corners = to_scene(vertices.reshape(-1, 3)).reshape(-1, 3, 3)
    normal = np.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0])
    facing = np.einsum("ij,ij->i", normal, centre - corners.mean(axis=1)) > 0
    return {"voxel_size": result["voxel"], "dims": [int(d) for d in result["dims"]], "triangles": int(len(faces)), "points": int(len(points)),
            "valid_cells": float(cells.mean()), "mean_distance_voxels": float(distance.mean()), "max_distance_voxels": float(distance.max()),
            "normals_facing_cameras": float(facing.mean())}


def test_the_depth_map_app_reports_what_the_definition_gives():
    from apps import depth_maps as app

    report = app.run(views=5, height=48, width=64, depths=33, smooth=cases.SMOOTHNESS)
    sc = cases.app_scene()
    scene = app.two_plane_scene(5, 48, 64, 2, 4.0)
    assert np.array_equal(scene["images"], sc["images"]) and np.array_equal(scene["poses"], sc["poses"]) and np.array_equal(scene["K"], sc["K"])
    assert (report["views"], report["height"], report["width"], report["depths"], report["from_model"]) == (5, 48, 64, 33, False)
    smoothed = report.pop("smoothed")
    assert (smoothed.pop("p1"), smoothed.pop("p2")) == cases.SMOOTHNESS
    for got, smoothness in ((report, None), (smoothed, cases.SMOOTHNESS)):
        want = depth_map_figures(sc, cases.chain(sc, smoothness), sc["depth"])
        assert {k: got[k] for k in want} == want, smoothness
    # the figures are those the definition's counts are pinned for
    inner = 42 * 58
    assert round(sum(r["within_one_before"] for r in report["per_view"]) * inner) == sweep_cases.TWO_PLANE_RIGHT_BEFORE
    assert round(sum(r["within_one_before"] for r in smoothed["per_view"]) * inner) == sgm_cases.TWO_PLANE_SGM[0]


def test_the_fusion_app_reports_what_the_definition_gives(tmp_path):
    from apps import fuse_depth_maps as app

    path = tmp_path / "surface.ply"
    report = app.run(views=5, height=48, width=64, depths=33, smooth=cases.SMOOTHNESS, ply=str(path))
    sc = cases.app_scene()
    smoothed = report.pop("smoothed")
    assert (smoothed.pop("p1"), smoothed.pop("p2")) == cases.SMOOTHNESS and report["from_model"] is False
    for got, smoothness in ((report, None), (smoothed, cases.SMOOTHNESS)):
        want = surface_figures(sc, cases.chain(sc, smoothness), sc["poses"])
        assert {k: got[k] for k in want} == want, smoothness
    assert report["triangles"] > 3000 and report["mean_distance_voxels"] < 0.6 and report["normals_facing_cameras"] > 0.95
    with open(path, "rb") as f:
        data = f.read()
    header, body = data.split(b"end_header\n", 1)
    sizes = {line.split()[1]: int(line.split()[2]) for line in header.decode("ascii").splitlines() if line.startswith("element")}
    assert sizes == {"vertex": report["points"], "face": report["triangles"]}
    assert len(body) == sizes["vertex"] * 27 + sizes["face"] * 13   # three doubles and three bytes a point, a byte and three int32 a face
    face = np.frombuffer(body[sizes["vertex"] * 27:], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    assert np.all(face["n"] == 3) and face["v"].min() == 0 and face["v"].max() == report["points"] - 1


# ---- poses, ranges and sources from a sparse model -----------------------------------------------------------------------------------
# The app's default size.  At 72 x 96 with the default 3000 sparse points and 0.1 pixels of noise the sparse reconstruction registers
# 2 of the 5 views, and the app refuses to go on.
MODEL_SIZE = (120, 160)
MODEL_DEPTHS = 33
# How far the share of interior pixels within one hypothesis of the truth, before the filter and over all views, may fall from the
# exact poses to the model's (profiles/plane_sweep/README.md gives the measured shares of this run and the reason for the margin)
MODEL_MARGIN = 0.02


@functools.lru_cache(maxsize=None)
def sparse_model():
    from apps import depth_maps as app

    scene = app.two_plane_scene(5, *MODEL_SIZE, 2, 4.0)
    return scene, app.model_of(scene, 3000, 0.1, 2)


def model_scene():
    """The scene of the app in the gauge of its sparse model: poses, per-view depth ranges and sources from the model."""
    from structure_from_motion_amd.stereo.depth_maps import depth_hypotheses

    scene, model = sparse_model()
    z = np.stack([depth_hypotheses(model["near"][v], model["far"][v], MODEL_DEPTHS) for v in range(5)])
    return dict(images=scene["images"], K=scene["K"], poses=np.asarray(model["poses"], dtype=np.float64), depths=z, sources=model["sources"],
                refs=np.arange(5, dtype=np.int32), depth=scene["depth"] * model["scale"], gauge=None, scale=model["scale"], key=("model",))


def test_the_sparse_model_is_a_general_gauge():
    scene, model = sparse_model()
    poses = np.asarray(model["poses"])
    assert poses.shape == (5, 12) and model["sources"].shape == (5, 4) and (model["sources"] >= 0).all()
    assert np.all(model["near"] > 0) and np.all(model["far"] > model["near"]) and model["scale"] > 0 and model["scale"] != 1.0
    assert np.sum(poses[1:, :9] == 0.0) == 0 and np.all(poses[1:, 10] != 0.0)   # (view 0 fixes the gauge)


def test_sweep_and_filter_on_the_models_poses_are_the_definitions():
    dm, _ = _libs()
    sc = model_scene()
    want = cases.chain(sc)
    maps = device_maps(sc, None)
    assert_maps(maps, want["maps"], MAP_NAMES, "depth maps in the model's gauge")
    assert_kept(dm.filter_depth_maps(maps, sc["K"], sc["poses"], sc["sources"], *FILTER_ARGS), want["kept"], "filter in the model's gauge")


def test_the_apps_from_a_model_report_what_the_definition_gives(monkeypatch):
    from apps import depth_maps as app
    from apps import fuse_depth_maps as fuse_app

    scene, model = sparse_model()
    sc = model_scene()

    def same_model(again, points, noise_px, seed):   # the reconstruction once: the apps get the model the reference was made from
        assert np.array_equal(again["images"], scene["images"]) and (points, noise_px, seed) == (3000, 0.1, 2)
        return model

    monkeypatch.setattr(app, "model_of", same_model)
    monkeypatch.setattr(fuse_app, "model_of", same_model)
    size = dict(views=5, height=MODEL_SIZE[0], width=MODEL_SIZE[1], depths=MODEL_DEPTHS)
    report = app.run(**size, from_model=True)
    assert report["from_model"] is True and report["model"] == {"points": model["points"], "scale": model["scale"]}
    want = depth_map_figures(sc, cases.chain(sc), sc["depth"])
    assert {k: report[k] for k in want} == want
    surface = fuse_app.run(**size, from_model=True)
    want = surface_figures(sc, cases.chain(sc), scene["poses"], model["scale"])
    assert {k: surface[k] for k in want} == want
    # against the truth: not worse than with the exact poses by more than MODEL_MARGIN
    exact = app.run(**size)
    share = lambda r: float(np.mean([v["within_one_before"] for v in r["per_view"]]))   # noqa: E731
    print(f"within_one_before, mean over the views: exact poses {share(exact):.4f}, the model's {share(report):.4f}; "
          f"after the filter {np.mean([v['within_one_after'] for v in exact['per_view']]):.4f} and "
          f"{np.mean([v['within_one_after'] for v in report['per_view']]):.4f}; mesh mean distance "
          f"{surface['mean_distance_voxels']:.3f} voxels, model points {model['points']}, scale {model['scale']:.6f}")
    assert share(report) >= share(exact) - MODEL_MARGIN


# ---- the scan beyond 1024 tiles -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def large_sphere(raised):
    big = cases.RAISED_SPHERE if raised else cases.LARGE_SPHERE
    total, count = to.sphere_state(**big)
    return total, count, cases.extract_in_slabs(total, count, None, big["origin"], big["voxel_size"])


@pytest.mark.parametrize("raised,half", [(False, False), (False, True), (True, False)])
def test_extract_beyond_1024_scan_tiles(raised, half):
    """1038 tiles of 4096 cells: every thread of the scan's totals kernel then sums two tiles.  The sphere of LARGE_SPHERE ends at
    cell layer 135 of 162 and cell 1024 * 4096 lies in layer 159, so the tiles beyond it are empty there; RAISED_SPHERE, the same
    sphere 0.2 higher, has triangles on both sides of that cell."""
    big = cases.RAISED_SPHERE if raised else cases.LARGE_SPHERE
    total, count, want = large_sphere(raised)
    assert (162 ** 3 + 4095) // 4096 == 1038 > 1024 and want[2] == (cases.RAISED_SPHERE_TRIANGLES if raised else cases.LARGE_SPHERE_TRIANGLES)
    rows = want[2] // 2 if half else want[2]
    vertices, grey, found = fusion_tests.run_extract((total, count, None), big["origin"], big["voxel_size"], 1, rows)
    assert found == want[2] and grey is None
    assert to.same_bytes(vertices, want[0][:rows]), f"max_triangles {rows}: vertices differ"
    cell = np.floor((want[0].mean(axis=1) - (np.array(big["origin"]) + 0.5 * big["voxel_size"])) / big["voxel_size"]).astype(np.int64)
    linear = (cell[:, 2] * 162 + cell[:, 1]) * 162 + cell[:, 0]
    assert np.all(np.diff(linear) >= 0) and (linear < 1024 * 4096).sum() > 300000
    assert (linear >= 1024 * 4096).sum() == (3610 if raised else 0)


def test_extract_exactly_one_scan_tile():
    small = cases.ONE_TILE_SPHERE
    total, count = to.sphere_state(**small)
    assert 16 ** 3 == 4096
    full = fusion_tests.check_extract((total, count, None), small["origin"], small["voxel_size"])
    assert full[2] > 1000


# ---- semi-global smoothing: the two widest depth groups ------------------------------------------------------------------------------
@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("count", [129, 256])
def test_sgm_wide_depth_groups(count, paths):
    volume, depths = sgm_cases.random_volume((2, count, 9, 21), 80 + count)
    got, want = sgm_tests.check(volume, depths, paths=paths)
    # winners all over the depth range, with and without the parabola step
    assert len(np.unique(want["index"])) > 100 and (want["depth"] != depths[0][np.clip(want["index"], 0, count - 1)]).any()
    assert (want["depth"] == depths[0][np.clip(want["index"], 0, count - 1)]).any()
