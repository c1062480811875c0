"""The dense stage as one chain without a GPU: the chain of the three NumPy definitions on a general
camera and in a general gauge (tests/dense_chain_cases.py).  It is the reference of tests/test_gpu_dense_chain.py, which compares
the device with it as bytes, so everything that makes it worth comparing with is asserted here: the general scene is general, the
input faults that the arc scenes cannot see change every stage on it, the definition does not depend on the gauge, and its
figures against the rendered truth are pinned."""
import numpy as np
import pytest

import dense_chain_cases as cases
import plane_sweep_cases as sweep_cases
import plane_sweep_oracle as po
import sgm_cases
import tsdf_cases
import tsdf_oracle as to

# The figures of the definition on the general camera, pinned as tests/sgm_cases.py pins its counts.  GENERAL_CAMERA_*: the same
# hypotheses for every view (plane_sweep_cases.hypotheses), (right, wrong) before and after the filter, in the arc gauge and in
# GAUGE alike, the cameras untilted.  GENERAL: cases.scene(True), the cameras tilted, hypotheses per view, in GAUGE: the counts, the
# triangles of the mesh and the mean and largest distance of its welded points to the true planes in voxels (the volume is laid along the gauge's axes, so these
# differ between gauges; the sums behind them run in NumPy's order, hence a relative 1e-9 and not the bytes).
GENERAL_CAMERA_SWEEP, GENERAL_CAMERA_SWEEP_FILTERED = (10939, 1133), (9568, 280)
GENERAL_CAMERA_SGM, GENERAL_CAMERA_SGM_FILTERED = (11533, 539), (10679, 174)
GENERAL = {None: dict(before=(11179, 832), after=(9747, 190), triangles=5592, mean_distance=0.5013430026287252,
                      max_distance=4.270653314090142),
           cases.SMOOTHNESS: dict(before=(11439, 572), after=(10361, 178), triangles=5902, mean_distance=0.49024877611767537,
                                  max_distance=4.219435634339827)}


def test_the_general_scene_is_general():
    sc = cases.scene(True)
    K, poses = sc["K"], sc["poses"]
    assert poses.shape == (5, 12) and not np.any(poses[:, :9] == 0.0) and not np.any(poses[:, 10] == 0.0)
    assert K[0, 1] != 0.0 and K[0, 0] != K[1, 1] and K[0, 2] != (64 - 1) / 2.0 and K[1, 2] != (48 - 1) / 2.0
    assert K[0, 2] != 64 / 2.0 and K[1, 2] != 48 / 2.0
    for pose in poses:   # still rotations, and the cameras are where they were
        R = pose[:9].reshape(3, 3)
        assert np.allclose(R @ R.T, np.eye(3), rtol=0, atol=1e-14) and np.linalg.det(R) > 0
    arc = cases.scene(False)
    centres = np.stack([-p[:9].reshape(3, 3).T @ p[9:] for p in poses])
    centres_arc = np.stack([-p[:9].reshape(3, 3).T @ p[9:] for p in arc["poses"]])
    assert np.allclose(cases.to_scene(centres, cases.GAUGE), centres_arc, rtol=0, atol=1e-13)
    # the rotation between two views is general as well: the sweep sees the poses through Rs Rr^T and ts - Rs Rr^T tr alone, which
    # no change of gauge makes general, so the cameras are tilted, each by its own roll and pitch
    for r in range(5):
        for v in range(5):
            if v != r:
                M = poses[v, :9].reshape(3, 3) @ poses[r, :9].reshape(3, 3).T
                assert np.abs(M).min() > 1e-3 and M[1, 1] < 1.0 - 1e-4
    assert len({float(t) for t in poses[:, 10]}) == 5
    # the hypotheses differ from view to view, and the arc scene is what the issue says of it
    assert len({z.tobytes() for z in sc["depths"]}) == 5
    assert int(np.sum(arc["poses"][:, :9] == 0.0)) == 22 and np.all(arc["poses"][:, 4] == 1.0) and np.all(arc["poses"][:, 10] == 0.0)
    assert arc["K"][0, 0] == arc["K"][1, 1] and arc["K"][0, 1] == 0.0


@pytest.mark.parametrize("name", list(cases.MUTATIONS))
def test_the_old_gap_is_real_and_the_general_scene_closes_it(name):
    mutate = cases.MUTATIONS[name]
    arc = cases.scene(False)
    K, poses = mutate(arc["K"], arc["poses"])
    if name in cases.INVISIBLE_ON_THE_ARC:   # the arc scene could not see it: the inputs are the same bytes
        assert np.array_equal(K, arc["K"]) and np.array_equal(poses, arc["poses"])
    else:
        assert not np.array_equal(poses, arc["poses"])
    sc = cases.scene(True)
    base = cases.chain(sc)
    K, poses = mutate(sc["K"], sc["poses"])
    assert not (np.array_equal(K, sc["K"]) and np.array_equal(poses, sc["poses"]))
    # each stage alone on the mutated K and poses, its other inputs those of the unmutated chain
    index = cases.sweep(cases.with_inputs(sc, K=K, poses=poses))["index"]
    for v in range(5):
        assert not np.array_equal(index[v], base["sweep"]["index"][v]), f"{name}: the sweep of view {v} does not see it"
    count = po.filter_depth_maps(base["maps"]["depth"], K, poses, sc["refs"], sc["sources"], **sweep_cases.TWO_PLANE_FILTER)["count"]
    for v in range(5):
        assert not np.array_equal(count[v], base["kept"]["count"][v]), f"{name}: the filter of view {v} does not see it"
    fused = to.integrate(tsdf_cases.empty_state(base["dims"]), base["kept"]["filtered"], sc["images"], K, poses, sc["refs"], base["origin"],
                         base["voxel"], base["truncation"])
    assert not np.array_equal(fused[1], base["fused"][1]), f"{name}: the integration does not see it"


@pytest.mark.parametrize("camera,tilt,per_view", [(False, False, False), (False, False, True), (True, False, False), (True, False, True),
                                                  (True, True, True)])
def test_the_definition_does_not_depend_on_the_gauge(camera, tilt, per_view):
    a = cases.scene(False, camera=camera, tilt=tilt, per_view=per_view)
    b = cases.scene(False, camera=camera, tilt=tilt, gauge=True, per_view=per_view)
    s = cases.GAUGE[2]
    assert np.array_equal(a["images"], b["images"]) and not np.array_equal(a["poses"], b["poses"])
    for smoothness in (None, cases.SMOOTHNESS):
        ra, rb = cases.chain(a, smoothness), cases.chain(b, smoothness)
        same = ra["maps"]["index"] == rb["maps"]["index"]
        kept_a, kept_b = np.isfinite(ra["kept"]["filtered"]), np.isfinite(rb["kept"]["filtered"])
        # at most 0.1 % of the pixels: a condition; the definition met it with 0 differing pixels
        assert (~same).sum() <= 0.001 * same.size and (kept_a != kept_b).sum() <= 0.001 * same.size
        has = same & (ra["maps"]["index"] >= 0)
        assert np.allclose(rb["maps"]["depth"][has] / s, ra["maps"]["depth"][has], rtol=1e-9, atol=0)
        fa, fb = cases.figures(a, ra), cases.figures(b, rb)
        assert (fa["before"], fa["after"]) == (fb["before"], fb["after"])
        if not camera and not tilt and not per_view:   # what the project already pins for this scene
            pinned = ((sweep_cases.TWO_PLANE_RIGHT_BEFORE, sweep_cases.TWO_PLANE_WRONG_BEFORE),
                      (sweep_cases.TWO_PLANE_RIGHT_AFTER, sweep_cases.TWO_PLANE_WRONG_AFTER)) if smoothness is None else \
                (sgm_cases.TWO_PLANE_SGM, sgm_cases.TWO_PLANE_SGM_FILTERED)
            assert (fa["before"], fa["after"]) == pinned and (fb["before"], fb["after"]) == pinned
        if camera and not tilt and not per_view:
            pinned = (GENERAL_CAMERA_SWEEP, GENERAL_CAMERA_SWEEP_FILTERED) if smoothness is None else \
                (GENERAL_CAMERA_SGM, GENERAL_CAMERA_SGM_FILTERED)
            assert (fa["before"], fa["after"]) == pinned and (fb["before"], fb["after"]) == pinned
        # the surface is where the planes are in either gauge: half a voxel on average, the stair of the occlusion edge at most
        for f in (fa, fb):
            assert f["triangles"] > 3000 and f["mean_distance"] < 0.6 and f["max_distance"] < 4.6


@pytest.mark.parametrize("smoothness", [None, cases.SMOOTHNESS])
def test_pinned_figures_on_the_general_scene(smoothness):
    sc = cases.scene(True)
    got = cases.figures(sc, cases.chain(sc, smoothness))
    want = GENERAL[smoothness]
    assert (got["before"], got["after"], got["triangles"]) == (want["before"], want["after"], want["triangles"])
    assert got["mean_distance"] == pytest.approx(want["mean_distance"], rel=1e-9, abs=0)
    assert got["max_distance"] == pytest.approx(want["max_distance"], rel=1e-9, abs=0)


def test_the_chain_with_and_without_grey_is_one_surface():
    sc = cases.scene(True)
    grey, plain = cases.chain(sc, None, True), cases.chain(sc, None, False)
    assert plain["fused"][2] is None and plain["mesh"][1] is None and grey["mesh"][1] is not None
    assert to.same_bytes(grey["mesh"][0], plain["mesh"][0]) and to.same_bytes(grey["fused"][0], plain["fused"][0])
    assert np.all(grey["fused"][3] == 0) and np.all(grey["sweep"]["status"] == 0) and np.all(grey["kept"]["status"] == 0)
    shade = grey["mesh"][1]
    assert np.all((shade >= 0.0) & (shade <= 255.0)) and shade.std() > 10


@pytest.mark.parametrize("layers", [4, 16])
def test_slabs_of_a_dyadic_grid_are_the_bytes_of_the_whole(layers):
    """The large GPU case compares with ``extract_in_slabs``; on 20^3 the same grid family is cheap enough to take whole."""
    dims, s, origin = (20, 20, 20), 2.0 ** -4, (-0.625,) * 3
    total, count = to.sphere_state(dims, s, origin, cases.LARGE_SPHERE["centre"], cases.LARGE_SPHERE["radius"])
    grey = (np.arange(total.size, dtype=np.int32).reshape(total.shape) * 7) % 256
    whole = to.extract_mesh(total, count, grey, origin, s)
    parts = cases.extract_in_slabs(total, count, grey, origin, s, layers=layers)
    assert whole[2] == parts[2] > 1000 and to.same_bytes(whole[0], parts[0]) and to.same_bytes(whole[1], parts[1])
    plain = cases.extract_in_slabs(total, count, None, origin, s, layers=layers)
    assert plain[1] is None and to.same_bytes(whole[0], plain[0])
    # the grid of the large case itself: every centre of it is exact, which is what makes a slab's centres those of the whole
    big = cases.LARGE_SPHERE
    cz = to.centres(big["dims"], big["origin"], big["voxel_size"])[2]
    for k0 in range(0, 162, 16):
        assert np.array_equal(to.centres((1, 1, 163 - k0), (0.0, 0.0, big["origin"][2] + k0 * big["voxel_size"]), big["voxel_size"])[2], cz[k0:])


def test_the_one_tile_sphere_has_exactly_one_tile_of_cells():
    small = cases.ONE_TILE_SPHERE
    total, count = to.sphere_state(**small)
    assert total.shape == (17, 17, 17) and 16 ** 3 == 4096
    found = to.extract_mesh(total, count, None, small["origin"], small["voxel_size"])[2]
    assert found > 1000
