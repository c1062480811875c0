"""What the host and GPU tests of the dense stage as one chain share (tests/test_dense_chain_host.py, tests/test_gpu_dense_chain.py;
DESIGN.md §6ai, §6aj, §6ak): the two-plane scene under a general camera and in a general gauge, the chain of the three NumPy
definitions from images to a mesh, and its figures.

The scenes of tests/plane_sweep_cases.py stand on an arc about the Y axis under a camera with fx == fy and no skew: 22 of the 45
rotation entries of five views are exactly zero, R[1][1] is 1 and t_y is 0, so a transposed off-axis entry of R, fx in the place
of fy, a wrong skew term of K^-1 or a dropped t_y changes nothing there.  Here the same world is described in other coordinates,
X' = s Rg X + tg: the images stay as they are, every pose becomes R' = R Rg^T, t' = s t - R' tg, every depth s times as large, and
no entry of any R' is zero.  The general camera has fx != fy, a skew and a principal point off the centre.

A change of gauge alone leaves the rotation between two views, Rs Rr^T, a rotation about Y, and gives every view the same t_y: the
sweep, which sees the poses through Rs Rr^T and ts - Rs Rr^T tr alone, would still not notice a dropped t_y or a transposed
off-axis entry of that product.  So the general scene also tilts every camera by a roll and a pitch of its own (``tilted``) and is
rendered anew from those cameras."""
import numpy as np

import plane_sweep_cases as sweep_cases
import plane_sweep_oracle as po
import sgm_oracle as so
import tsdf_cases
import tsdf_oracle as to

VIEWS, HEIGHT, WIDTH, DEPTHS, RADIUS, TOP_K, SOURCES = 5, 48, 64, 33, 3, 2, 4
SMOOTHNESS = (0.1, 0.8)
PIXELS, TRUNCATION_VOXELS, MIN_COUNT = 2.0, 4.0, 2          # the fusion settings of apps/fuse_depth_maps.py


def _rotation(axis, angle):
    """Rodrigues' formula."""
    k = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(angle) * Kx + (1.0 - np.cos(angle)) * (Kx @ Kx)


# (Rg, tg, s): 0.3 rad about (0.2, -0.5, 0.8), a translation and a scale
GAUGE = (_rotation((0.2, -0.5, 0.8), 0.3), np.array([0.3, -1.0, 2.0]), 1.7)


# (roll about the optical axis, pitch about the camera's x axis) of each view in degrees: with them the rotation between two views
# is no rotation about Y either, and the up vectors of the cameras differ
TILT_DEG = ((-6.0, 1.5), (3.5, -2.0), (-2.0, 2.5), (5.0, -1.0), (-4.5, 2.0))


def tilted(poses):
    """The cameras of ``poses`` at the same centres, each rolled and pitched by its entry of TILT_DEG: R' = Rz Rx R, t' = Rz Rx t."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 12)
    out = np.empty_like(poses)
    for v, pose in enumerate(poses):
        roll, pitch = np.radians(TILT_DEG[v % len(TILT_DEG)])
        T = _rotation((0.0, 0.0, 1.0), roll) @ _rotation((1.0, 0.0, 0.0), pitch)
        out[v, :9], out[v, 9:] = (T @ pose[:9].reshape(3, 3)).reshape(9), T @ pose[9:]
    return out


def general_camera(height, width):
    """fx != fy, a skew of 4 and a principal point off the centre."""
    return np.array([[1.3 * width, 4.0, width / 2.0 - 3.5], [0.0, 1.05 * width, height / 2.0 + 2.25], [0.0, 0.0, 1.0]])


def regauge(poses, gauge):
    """The poses (V, 12) of the same cameras in the coordinates X' = s Rg X + tg: R' = R Rg^T, t' = s t - R' tg."""
    Rg, tg, s = gauge
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 12)
    out = np.empty_like(poses)
    for v, pose in enumerate(poses):
        R = pose[:9].reshape(3, 3) @ Rg.T
        out[v, :9], out[v, 9:] = R.reshape(9), s * pose[9:] - R @ tg
    return out


def to_scene(points, gauge):
    """Points (N, 3) of the gauge's coordinates in the scene's: X = Rg^T (X' - tg) / s; ``gauge`` None: as they are."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    if gauge is None:
        return points
    Rg, tg, s = gauge
    return (points - tg) @ Rg / s


_SCENES = {}


def scene(general, camera=None, gauge=None, tilt=None, per_view=True, shape=(HEIGHT, WIDTH), views=VIEWS, seed=2, depths=DEPTHS, sources=SOURCES):
    """The two-plane scene of ``plane_sweep_cases.scene(48, 64, views=5, seed=2, two_planes=True)``; with ``general`` rendered by
    ``general_camera`` from cameras tilted by ``TILT_DEG`` and its poses moved into ``GAUGE`` (``camera``, ``tilt`` and ``gauge``,
    three bools, choose each alone; the images do not depend on ``gauge``).  ``depth``, the
    truth, is in the gauge's scale for comparisons only.  The hypotheses differ from view to view (``per_view``; else the ones
    of plane_sweep_cases.hypotheses for every view).  -> dict(images, depth, K, poses, depths (V, D), sources, refs, gauge (or
    None), scale, key); computed once, never written."""
    camera, gauge, tilt = (general if camera is None else camera), (general if gauge is None else gauge), (general if tilt is None else tilt)
    key = (bool(camera), bool(gauge), bool(tilt), bool(per_view), tuple(shape), views, seed, depths, sources)
    if key not in _SCENES:
        from structure_from_motion_amd import synthetic
        from structure_from_motion_amd.stereo.depth_maps import depth_hypotheses

        H, W = shape
        arc = sweep_cases.scene(H, W, views=views, seed=seed, two_planes=True)
        sc, own = dict(arc), (tilted(arc["poses"]) if tilt else arc["poses"])
        if camera or tilt:
            u, v = sweep_cases._slant(25.0)
            planes = [((0.0, 0.0, 5.0), u, v, None), ((0.1, 0.0, 3.6), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.45, 0.5))]
            sc = synthetic.plane_views(H, W, own, planes, seed=seed, K=general_camera(H, W) if camera else None)
            sc["near"], sc["far"] = float(np.nanmin(sc["depth"]) / 1.05), float(np.nanmax(sc["depth"]) * 1.05)
        s = GAUGE[2] if gauge else 1.0
        if per_view:
            z = np.stack([depth_hypotheses(sc["near"] * (1.0 - 0.01 * v), sc["far"] * (1.0 + 0.01 * v), depths) for v in range(views)])
        else:
            z = np.broadcast_to(depth_hypotheses(sc["near"], sc["far"], depths), (views, depths))
        sc.update(poses=regauge(own, GAUGE) if gauge else own, depth=sc["depth"] * s, depths=np.ascontiguousarray(z * s),
                  sources=sweep_cases.nearest_sources(views, sources), refs=np.arange(views, dtype=np.int32), gauge=GAUGE if gauge else None,
                  scale=s, key=key)
        _SCENES[key] = sc
    return _SCENES[key]


def small_scene():
    """The general scene at 37 x 45 with 4 views, D = 5 and S = 3 (radius 2): ragged against the sweep's tiles."""
    return scene(True, shape=(37, 45), views=4, seed=12, depths=5, sources=3)


def app_scene(height=HEIGHT, width=WIDTH, depths=DEPTHS):
    """The scene of ``apps.depth_maps.run(views=5, height, width, depths)`` with exact poses: the arc, the default camera, the
    same hypotheses for every view."""
    return scene(False, per_view=False, shape=(height, width), depths=depths)


def with_inputs(sc, **change):
    """The scene with other inputs (K, poses, ...): not cached by ``chain``."""
    return {**sc, **change, "key": None}


# ---- the chain of the definitions ----------------------------------------------------------------------------------------------------
_SWEEPS, _CHAINS = {}, {}


def sweep(sc, radius=RADIUS, top_k=TOP_K, min_sources=1):
    key = None if sc["key"] is None else (sc["key"], radius, top_k, min_sources)
    if key is None or key not in _SWEEPS:
        out = po.plane_sweep(sc["images"], sc["K"], sc["poses"], sc["refs"], sc["sources"], sc["depths"], radius, top_k, min_sources)
        if key is None:
            return out
        _SWEEPS[key] = out
    return _SWEEPS[key]


def volume_of(kept_depth, kept_points, sc, pixels=PIXELS, truncation_voxels=TRUNCATION_VOXELS):
    """(voxel size, truncation, origin (3,), dims (3,)) as apps/fuse_depth_maps.py and ``fusion.fuse_depth_maps`` lay the volume
    around the kept points: the host functions of stereo/fusion.py on the definition's filter outputs."""
    from structure_from_motion_amd.stereo import fusion

    filtered = filtered_maps(kept_depth, kept_points, sc)
    voxel = fusion.suggest_voxel_size(filtered, sc["K"], pixels)
    truncation = truncation_voxels * voxel
    low, high = fusion.volume_bounds(filtered, truncation)
    dims = np.maximum(np.ceil((high - low) / voxel).astype(np.int64), 2)
    return voxel, truncation, low, dims


def filtered_maps(kept_depth, kept_points, sc, count=None):
    from structure_from_motion_amd.stereo.depth_maps import FilteredDepthMaps

    count = np.zeros(kept_depth.shape, dtype=np.int32) if count is None else count
    return FilteredDepthMaps(kept_depth, count, kept_points, np.arange(len(kept_depth)), sc["images"])


def chain(sc, smoothness=None, with_grey=True, filter_args=None, radius=RADIUS, top_k=TOP_K):
    """The definitions from the images to the mesh, nothing new: po.plane_sweep -> so.sgm_aggregate (with ``smoothness`` =
    (p1, p2): 8 paths, invalid cost 1) -> po.filter_depth_maps -> fusion.suggest_voxel_size / volume_bounds -> to.integrate ->
    to.extract_mesh.  -> dict(sweep, smooth (or None), maps (depth, index, cost: the smoothed ones, or the sweep's), kept,
    voxel, truncation, origin, dims, fused (sum, count, grey_sum, status), mesh (vertices, grey, triangles))."""
    filter_args = dict(sweep_cases.TWO_PLANE_FILTER if filter_args is None else filter_args)
    key = None if sc["key"] is None else (sc["key"], smoothness, with_grey, tuple(sorted(filter_args.items())), radius, top_k)
    if key is not None and key in _CHAINS:
        return _CHAINS[key]
    swept = sweep(sc, radius, top_k)
    smooth = None if smoothness is None else so.sgm_aggregate(swept["volume"], sc["depths"], smoothness[0], smoothness[1], 1.0, 8)
    maps = {name: (swept if smooth is None else smooth)[name] for name in ("depth", "index", "cost")}
    kept = po.filter_depth_maps(maps["depth"], sc["K"], sc["poses"], sc["refs"], sc["sources"], **filter_args)
    voxel, truncation, origin, dims = volume_of(kept["filtered"], kept["points"], sc)
    fused = to.integrate(tsdf_cases.empty_state(dims, with_grey), kept["filtered"], sc["images"] if with_grey else None, sc["K"], sc["poses"],
                         sc["refs"], origin, voxel, truncation)
    mesh = to.extract_mesh(*fused[:3], origin, voxel, MIN_COUNT)
    out = dict(sweep=swept, smooth=smooth, maps=maps, kept=kept, voxel=voxel, truncation=truncation, origin=origin, dims=dims, fused=fused,
               mesh=mesh)
    if key is not None:
        _CHAINS[key] = out
    return out


def truth_index(sc):
    """The hypothesis of its view nearest to the true depth of every pixel, in inverse depth; -1 where no plane was hit."""
    with np.errstate(all="ignore"):
        index = np.abs(1.0 / sc["depth"][..., None] - 1.0 / sc["depths"][:, None, None, :]).argmin(axis=-1)
    return np.where(np.isfinite(sc["depth"]), index, -1)


def figures(sc, result, radius=RADIUS):
    """-> dict(before, after: (right, wrong) of plane_sweep_cases.within_one for the chain's maps, all of them and those the filter
    kept; triangles; mean_distance, max_distance: of the welded mesh points, brought into the scene, to the nearest true plane
    (apps.fuse_depth_maps.distance_to_planes), in voxels)."""
    from apps.fuse_depth_maps import distance_to_planes
    from structure_from_motion_amd.stereo import fusion

    truth, index = truth_index(sc), result["maps"]["index"]
    points, _, _ = fusion.Mesh(result["mesh"][0]).weld()
    distance = distance_to_planes(to_scene(points, sc["gauge"])) / (result["voxel"] / sc["scale"])
    return dict(before=sweep_cases.within_one(index, truth, np.ones(index.shape, dtype=bool), radius),
                after=sweep_cases.within_one(index, truth, np.isfinite(result["kept"]["filtered"]), radius),
                triangles=int(result["mesh"][2]), mean_distance=float(distance.mean()), max_distance=float(distance.max()))


# ---- the input mutations that the arc scene cannot see --------------------------------------------------------------------------------
def _no_skew(K, poses):
    K = K.copy()
    K[0, 1] = 0.0
    return K, poses


def _fy_is_fx(K, poses):
    K = K.copy()
    K[1, 1] = K[0, 0]
    return K, poses


def _no_ty(K, poses):
    poses = poses.copy()
    poses[:, 10] = 0.0
    return K, poses


def _first_rotation_transposed(K, poses):
    poses = poses.copy()
    poses[0, :9] = poses[0, :9].reshape(3, 3).T.reshape(9)
    return K, poses


# name -> (K, poses) -> (K, poses); the first three are the identity on the arc scene
MUTATIONS = {"skew := 0": _no_skew, "fy := fx": _fy_is_fx, "t_y := 0": _no_ty, "R of view 0 transposed": _first_rotation_transposed}
INVISIBLE_ON_THE_ARC = ("skew := 0", "fy := fx", "t_y := 0")


# ---- the scan beyond 1024 tiles -------------------------------------------------------------------------------------------------------
# 163^3 voxels: 162^3 = 4 251 528 cells, 1038 scan tiles of 4096; a dyadic grid (voxel 2^-7, origin -0.625), on which every centre
# o + (i + 0.5) s is exact, so the centres of a slab taken alone are the bytes of the same centres in the whole volume
LARGE_SPHERE = dict(dims=(163, 163, 163), voxel_size=2.0 ** -7, origin=(-0.625,) * 3, centre=(0.013, 0.018, 0.021), radius=0.4173)
LARGE_SPHERE_TRIANGLES = 321832
# that sphere lies below cell 1024 * 4096 (cell layer 159 of 162); 0.2 higher it reaches the last layer
RAISED_SPHERE = dict(LARGE_SPHERE, centre=(0.013, 0.018, 0.2213))
RAISED_SPHERE_TRIANGLES = 321848
ONE_TILE_SPHERE = dict(dims=(17, 17, 17), voxel_size=2.0 ** -4, origin=(-0.625,) * 3, centre=(-0.087, -0.082, -0.079), radius=0.4173)


def extract_in_slabs(total, count, grey_sum, origin, voxel_size, min_count=1, layers=16):
    """``to.extract_mesh`` of the whole volume, taken over slabs of ``layers`` cell layers in z and joined: the cells of a slab
    are those of voxel layers k0 .. k0 + layers, and a cell's triangles come in the order of the whole, as z is the slowest
    index.  The bytes of the whole on a dyadic grid only, where ``origin_z + k0 * voxel_size`` and every centre are exact."""
    nz = total.shape[0]
    parts, found = [], 0
    for k0 in range(0, nz - 1, layers):
        k1 = min(k0 + layers, nz - 1) + 1
        low = (origin[0], origin[1], origin[2] + k0 * voxel_size)
        part = to.extract_mesh(total[k0:k1], count[k0:k1], None if grey_sum is None else grey_sum[k0:k1], low, voxel_size, min_count)
        parts.append(part)
        found += part[2]
    vertices = np.concatenate([p[0] for p in parts])
    grey = None if grey_sum is None else np.concatenate([p[1] for p in parts])
    return vertices, grey, found
