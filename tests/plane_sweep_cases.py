"""What the host and GPU tests of the dense stage share (tests/test_plane_sweep_host.py, tests/test_gpu_plane_sweep.py;
csrc/sfm_plane_sweep.hip): the rendered scenes, the accuracy counts of the definition and the stream case of
``sfm_plane_sweep`` and ``sfm_filter_depth_maps``."""
import functools

import numpy as np

import plane_sweep_oracle as po
import stream_cases

OK, BAD_REFERENCE = 0, 1
SWEEP_NAMES = ("depth", "index", "cost", "status", "volume")
FILTER_NAMES = ("count", "filtered", "points", "status")

# The accuracy of the definition itself (tests/test_plane_sweep_host.py computes both on the CPU; DESIGN.md §6ai quotes them).
# SLANTED_*: a plane slanted by 25 degrees, 5 views of 48 x 64, D = 33, radius 3, four sources: the interior pixels (at least
# `radius` from the border) of all views whose winner lies within one hypothesis of the truth, out of SLANTED_INTERIOR.
# TWO_PLANE_*: a bounded plane in front of a slanted one, top_k = 2, then the filter (one pixel, 2 % of the depth, two agreeing
# sources; a hypothesis step is 2.3 % of the depth here): the interior
# pixels kept and within one hypothesis, and the kept ones that are further off, before (the raw winners) and after.
SLANTED_INTERIOR = 5 * 42 * 58
SLANTED_WITHIN_ONE = 11473
TWO_PLANE_RIGHT_BEFORE, TWO_PLANE_WRONG_BEFORE = 10837, 1231
TWO_PLANE_RIGHT_AFTER, TWO_PLANE_WRONG_AFTER = 9282, 383
TWO_PLANE_FILTER = dict(max_pixel_error=1.0, max_relative_depth_error=0.02, min_consistent=2)


def _slant(degrees):
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    return (c, 0.0, s), (0.0, 1.0, 0.0)


@functools.lru_cache(maxsize=None)
def scene(height, width, views=4, seed=1, two_planes=False, step_deg=4.0):
    """A rendered scene (computed once, never written): ``views`` cameras on an arc, a plane slanted by 25 degrees through
    (0, 0, 5) and, with ``two_planes``, a bounded fronto-parallel plane at depth 3.6 in front of it.  -> dict(images, depth (the
    truth), K, poses, near, far)."""
    from structure_from_motion_amd import synthetic

    poses = synthetic.arc_poses(views, step_deg, 5.0)
    u, v = _slant(25.0)
    planes = [((0.0, 0.0, 5.0), u, v, None)]
    if two_planes:
        planes.append(((0.1, 0.0, 3.6), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.45, 0.5)))
    out = synthetic.plane_views(height, width, poses, planes, seed=seed)
    out["poses"] = poses
    out["near"], out["far"] = float(np.nanmin(out["depth"]) / 1.05), float(np.nanmax(out["depth"]) * 1.05)
    return out


def nearest_sources(views, count, refs=None):
    """(R, count) int32: the nearest view indices of each reference, -1 where there are not enough."""
    refs = range(views) if refs is None else refs
    rows = []
    for r in refs:
        order = sorted((v for v in range(views) if v != r), key=lambda v: (abs(v - r), v))[:count]
        rows.append(order + [-1] * (count - len(order)))
    return np.array(rows, dtype=np.int32).reshape(len(rows), count)


def hypotheses(sc, count):
    from structure_from_motion_amd.stereo.depth_maps import depth_hypotheses

    return depth_hypotheses(sc["near"], sc["far"], count)


def truth_index(sc, z):
    """The hypothesis nearest to the true depth of every pixel, in inverse depth; -1 where no plane was hit."""
    with np.errstate(all="ignore"):
        index = np.abs(1.0 / sc["depth"][..., None] - 1.0 / z).argmin(axis=-1)
    return np.where(np.isfinite(sc["depth"]), index, -1)


def interior(shape, radius):
    mask = np.zeros(shape, dtype=bool)
    mask[..., radius:shape[-2] - radius, radius:shape[-1] - radius] = True
    return mask


def within_one(index, truth, keep, radius):
    """(right, wrong): the interior pixels of ``keep`` whose hypothesis lies within one of the truth, and the others of ``keep``."""
    at = keep & interior(index.shape, radius) & (index >= 0)
    right = at & (truth >= 0) & (np.abs(index - truth) <= 1)
    return int(right.sum()), int((at & ~right).sum())


@functools.lru_cache(maxsize=None)
def slanted_accuracy():
    """The oracle on the slanted plane: -> (sweep outputs, truth index, hypotheses)."""
    sc = scene(48, 64, views=5, seed=1)
    z = hypotheses(sc, 33)
    out = po.plane_sweep(sc["images"], sc["K"], sc["poses"], np.arange(5), nearest_sources(5, 4), np.broadcast_to(z, (5, 33)), 3)
    return out, truth_index(sc, z), z


@functools.lru_cache(maxsize=None)
def two_plane_accuracy():
    """The oracle on the two-plane scene, sweep (top_k = 2) and filter (TWO_PLANE_FILTER): -> (sweep, filter, truth index)."""
    sc = scene(48, 64, views=5, seed=2, two_planes=True)
    z = hypotheses(sc, 33)
    sources = nearest_sources(5, 4)
    sweep = po.plane_sweep(sc["images"], sc["K"], sc["poses"], np.arange(5), sources, np.broadcast_to(z, (5, 33)), 3, top_k=2)
    kept = po.filter_depth_maps(sweep["depth"], sc["K"], sc["poses"], np.arange(5), sources, **TWO_PLANE_FILTER)
    return sweep, kept, truth_index(sc, z)


def sweep_inputs(sc, depth_count, source_count, refs=None):
    """The arrays of a sweep call on a scene: dict(images, K (9,), poses, refs, sources, depths)."""
    V = len(sc["images"])
    refs = np.arange(V, dtype=np.int32) if refs is None else np.asarray(refs, dtype=np.int32)
    z = hypotheses(sc, depth_count)
    return dict(images=sc["images"], K=np.ascontiguousarray(sc["K"].reshape(9)), poses=np.ascontiguousarray(sc["poses"]), refs=refs,
                sources=nearest_sources(V, source_count, [int(r) % V for r in refs]),
                depths=np.ascontiguousarray(np.broadcast_to(z, (len(refs), depth_count))))


# The op list is empty on purpose, as for register_views (tests/register_views_cases.py): tests/test_stream_cases_host.py requires
# every op a case names to be in ops.FUNCTIONAL_OPS / INPLACE_OPS, two tuples that an earlier schema guard pins, and the ops of
# these calls are listed in ops.DEPTH_MAP_OPS.  The calls below still go through them, and their outputs are compared.
@stream_cases.case(["sfm_plane_sweep", "sfm_filter_depth_maps"], [])
def plane_sweep(dev):
    """The sweep of four views of 37 x 45 (D = 9, S = 2, radius 2) and the filter on its depth maps, two scenes of equal shapes and
    different images: the C entry points on the test's buffers and workspace, and the functional ops on the same inputs."""
    import torch

    from structure_from_motion_amd import ops

    i = stream_cases.Inst(dev)
    # three spare streams of torch's pool beside this case: four in all, so that every later side stream of
    # tests/test_gpu_streams.py keeps its hardware queue (the comment in tests/register_views_cases.py)
    i.keep_alignment = [torch.cuda.Stream() for _ in range(3)]
    V, H, W, D, S, radius = 4, 37, 45, 9, 2, 2
    a, b = sweep_inputs(scene(H, W, V, seed=11), D, S), sweep_inputs(scene(H, W, V, seed=12), D, S)
    assert not np.array_equal(a["images"], b["images"])
    images = i.inp(a["images"], b["images"])
    # the hypotheses differ too, so that the homographies in the workspace do
    K, poses, depths = i.same(a["K"]), i.same(a["poses"]), i.inp(a["depths"], b["depths"] * 1.01)
    refs, sources = i.same(a["refs"], torch.int32), i.same(a["sources"], torch.int32)
    depth, index = i.out("depth", (V, H, W), torch.float64), i.out("index", (V, H, W), torch.int32)
    cost, status = i.out("cost", (V, H, W), torch.float64), i.out("status", (V,), torch.int32)
    volume = i.out("volume", (V, D, H, W), torch.float64)
    count, filtered = i.out("count", (V, H, W), torch.int32), i.out("filtered", (V, H, W), torch.float64)
    points, filter_status = i.out("points", (V, H, W, 3), torch.float64), i.out("filter_status", (V,), torch.int32)
    lib = stream_cases._lib()
    ws = i.work(lib.sfm_plane_sweep_workspace_bytes(V, H, W, V, S, D))
    i.constant |= {"status", "filter_status"}   # every reference is a view
    op = ops.load()

    def call():
        st = stream_cases._st()
        stream_cases._check(lib.sfm_plane_sweep(images.data_ptr(), V, H, W, K.data_ptr(), poses.data_ptr(), refs.data_ptr(), V,
                                                sources.data_ptr(), S, depths.data_ptr(), D, radius, 0, 1, 1.0, depth.data_ptr(),
                                                index.data_ptr(), cost.data_ptr(), status.data_ptr(), volume.data_ptr(), ws.data_ptr(),
                                                ws.numel(), st), "sfm_plane_sweep")
        stream_cases._check(lib.sfm_filter_depth_maps(depth.data_ptr(), V, H, W, K.data_ptr(), poses.data_ptr(), refs.data_ptr(), V,
                                                      sources.data_ptr(), S, 1.0, 0.01, 1, count.data_ptr(), filtered.data_ptr(),
                                                      points.data_ptr(), filter_status.data_ptr(), st), "sfm_filter_depth_maps")
        swept = op.plane_sweep(images, K, poses, refs, sources, depths, radius, 0, 1, 1.0, False)
        kept = op.filter_depth_maps(swept[0], K, poses, refs, sources, 1.0, 0.01, 1)
        return stream_cases.Returned(swept[:3] + kept[:3])   # (the statuses are the same in both scenes)
    i.call = call
    return i


def exact_camera():
    """A camera of powers of two: with the poses of the hand-made cases every product and quotient of the definition is exact."""
    return np.array([[64.0, 0.0, 16.0], [0.0, 64.0, 4.0], [0.0, 0.0, 1.0]])


def pose(R=None, t=(0.0, 0.0, 0.0)):
    return np.concatenate([np.eye(3).reshape(9) if R is None else np.asarray(R, dtype=np.float64).reshape(9), np.asarray(t, dtype=np.float64)])


def filter_boundary_case():
    """Two views of 8 x 40 whose reprojection errors are exact: view 1 is view 0 moved by half a unit in x.  A pixel of view 0 at
    depth 4 lands 8 pixels to the right in view 1; carried back with depth 2 it returns 8 pixels to the LEFT of where it started
    at depth 2: a pixel error of exactly 8 and a depth error of exactly 2 = 0.5 * 4.  -> dict(depth (2, 8, 40), K, poses, refs,
    sources, on_boundary (y, x), beyond (y, x), hole (y, x)): at ``beyond`` the source depth is 2 / (1 + 2^-30), so the error is
    just above 8; the source pixel of ``hole`` has no depth."""
    H, W = 8, 40
    depth = np.full((2, H, W), np.nan)
    depth[0, :, :24] = 4.0
    depth[1] = 2.0
    on_boundary, beyond, hole = (3, 5), (3, 9), (5, 11)
    depth[1, beyond[0], beyond[1] + 8] = 2.0 / (1.0 + 2.0 ** -30)
    depth[1, hole[0], hole[1] + 8] = np.nan
    return dict(depth=depth, K=exact_camera().reshape(9), poses=np.stack([pose(), pose(t=(0.5, 0.0, 0.0))]),
                refs=np.array([0, 1], dtype=np.int32), sources=np.array([[1], [0]], dtype=np.int32), on_boundary=on_boundary,
                beyond=beyond, hole=hole)
