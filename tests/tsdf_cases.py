"""What the host and GPU tests of the fusion share (tests/test_tsdf_fusion_host.py, tests/test_gpu_depth_fusion.py;
csrc/sfm_tsdf.hip): the scenes, the volumes and states of the extraction cases, the hand-made exact cases and the
stream case of ``sfm_tsdf_integrate`` and ``sfm_tsdf_extract_mesh``."""
import functools

import numpy as np

import plane_sweep_cases as sweep_cases
import stream_cases
import tsdf_oracle as to

OK, BAD_VIEW = 0, 1

# the slanted plane of the accuracy tests: 5 exact depth maps of 48 x 64, a volume of 23 x 18 x 22 voxels of 0.1
PLANE_DIMS, PLANE_ORIGIN, PLANE_VOXEL, PLANE_TRUNCATION = (23, 18, 22), (-1.2, -0.9, 3.9), 0.1, 0.4
PLANE_NORMAL = np.cross((np.cos(np.radians(25.0)), 0.0, np.sin(np.radians(25.0))), (0.0, 1.0, 0.0))
PLANE_POINT = np.array([0.0, 0.0, 5.0])
SPHERE = dict(dims=(12, 12, 12), voxel_size=0.25, origin=(-1.5, -1.5, -1.5), centre=(0.03, -0.02, 0.05), radius=0.9173)


def empty_state(dims, with_grey=True):
    shape = tuple(dims)[::-1]
    return np.zeros(shape), np.zeros(shape, dtype=np.int32), (np.zeros(shape, dtype=np.int32) if with_grey else None)


@functools.lru_cache(maxsize=None)
def plane_scene(seed=1):
    """The slanted plane seen by five views (computed once, never written)."""
    return sweep_cases.scene(48, 64, views=5, seed=seed)


@functools.lru_cache(maxsize=None)
def fused_plane(seed=1):
    """The oracle's state after all five exact depth maps of the slanted plane: -> (sum, count, grey_sum, status)."""
    sc = plane_scene(seed)
    return to.integrate(empty_state(PLANE_DIMS), sc["depth"], sc["images"], sc["K"], sc["poses"], np.arange(5), PLANE_ORIGIN, PLANE_VOXEL,
                        PLANE_TRUNCATION)


def plane_distance(vertices):
    """The distance of every vertex to the slanted plane, in voxels."""
    return np.abs((np.asarray(vertices).reshape(-1, 3) - PLANE_POINT) @ PLANE_NORMAL) / PLANE_VOXEL


def normals(vertices):
    return np.cross(vertices[:, 1] - vertices[:, 0], vertices[:, 2] - vertices[:, 0])


def weld(vertices):
    """(points, faces) of triangles whose equal corners (as bytes) are merged; NumPy only, apart from ``Mesh.weld``."""
    flat = np.ascontiguousarray(vertices.reshape(-1, 3))
    _, first, inverse = np.unique(flat.view(np.dtype((np.void, 24))).reshape(-1), return_index=True, return_inverse=True)
    return flat[first], inverse.reshape(-1, 3)


def directed_edges(faces):
    """{(a, b): how often the directed edge occurs}."""
    edges = {}
    for f in faces:
        for a, b in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0])):
            edges[(int(a), int(b))] = edges.get((int(a), int(b)), 0) + 1
    return edges


# ---- integration cases ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def integrate_scene():
    """Four views of 12 x 16 of the slanted plane: view 2 looks away, and the depth maps hold a NaN, an infinite, a zero and a
    negative block.  -> dict(depth, images, K (9,), poses)."""
    sc = sweep_cases.scene(12, 16, views=4, seed=21)
    depth, poses = sc["depth"].copy(), sc["poses"].copy()
    away = np.diag([-1.0, 1.0, -1.0])
    poses[2] = sweep_cases.pose(away @ poses[2, :9].reshape(3, 3), away @ poses[2, 9:])
    depth[0, 2:5, 3:7] = np.nan
    depth[1, 6:9, 2:6] = np.inf
    depth[1, 1:3, 10:14] = -np.inf
    depth[3, 4:8, 8:12] = 0.0
    depth[0, 7:10, 9:13] = -depth[0, 7:10, 9:13]
    return dict(depth=depth, images=sc["images"], K=np.ascontiguousarray(sc["K"].reshape(9)), poses=np.ascontiguousarray(poses))


def integrate_volume(dims):
    """(origin, voxel_size, truncation) of a volume about (0, 0, 5) that reaches beyond the images: 0.25 a voxel, wider than the
    frustum of a 12 x 16 image (2.1 by 1.6 units at depth 5) for the wide shapes."""
    s = 0.25
    return tuple(c - 0.5 * n * s for c, n in zip((0.05, -0.03, 5.02), dims)), s, 0.6


def exact_voxel_case():
    """One voxel, one view, every operation exact: the identity pose, a camera of powers of two (f = 64, c = (16, 4)) and the
    voxel centre (1 / 64, 0, 2).  u = 64 / 64 / 2 + 16 = 16.5, exactly half a pixel: x = floor(17.0) = 17; v = 4, z = 2.
    -> dict(dims, origin, voxel_size, truncation = 0.25, K, poses, pixel (y, x))."""
    return dict(dims=(1, 1, 1), origin=(1.0 / 64.0 - 0.25, -0.25, 1.75), voxel_size=0.5, truncation=0.25,
                K=sweep_cases.exact_camera().reshape(9), poses=sweep_cases.pose()[None], pixel=(4, 17))


def exact_column_case():
    """A column of 1 x 1 x 12 voxels on the optical axis of the exact camera, centres at z = 1.0 + k / 8, under a constant depth map
    of 2.0 with truncation 0.25: k = 10 has sdf = -0.25 = -truncation exactly (kept, f = -1), k = 11 is hidden, k = 6 has sdf =
    truncation exactly (f = 1), k = 8 lies on the surface (f = 0).  -> dict(dims, origin, voxel_size, truncation, K, poses, depth)."""
    return dict(dims=(1, 1, 12), origin=(-0.0625, -0.0625, 0.9375), voxel_size=0.125, truncation=0.25,
                K=sweep_cases.exact_camera().reshape(9), poses=sweep_cases.pose()[None], depth=np.full((1, 8, 40), 2.0))


# ---- extraction cases -----------------------------------------------------------------------------------------------------------------
def sphere_state():
    return to.sphere_state(**SPHERE)


def holes_state(dims=(9, 7, 6), seed=3):
    """A state as integration leaves it on a slanted surface, with counts of 0 to 3 so that min_count 1, 2 and 3 each leave other
    cells, and grey sums.  -> (sum, count, grey_sum, origin, voxel_size)."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    origin, s = (-0.4, 0.3, 1.1), 0.2
    cx, cy, cz = to.centres(dims, origin, s)
    count = rng.integers(0, 4, size=(nz, ny, nx)).astype(np.int32)
    count[1:4, 1:5, 2:7] = 3   # a block that every min_count keeps
    distance = (0.3 * cx[None, None, :] - 0.2 * cy[None, :, None] + cz[:, None, None] - 1.75) / 0.8
    total = np.clip(distance, -1.0, 1.0) * count + rng.normal(0.0, 0.01, size=count.shape) * (count > 0)
    grey = (rng.integers(0, 256, size=count.shape) * count).astype(np.int32)
    return total, count, grey, origin, s


def zero_corner_state():
    """A 4 x 3 x 3 volume whose values are small integers, several of them exactly zero (and one -0.0, which is not negative)."""
    rng = np.random.default_rng(5)
    total = rng.integers(-2, 3, size=(3, 3, 4)).astype(np.float64)
    total[1, 1, 1] = 0.0
    total[1, 1, 2] = -0.0
    total[0, 0, 0] = -1.0
    count = np.ones(total.shape, dtype=np.int32)
    return total, count, (np.arange(total.size, dtype=np.int32).reshape(total.shape) * 7) % 256, (0.0, 0.0, 0.0), 0.5


def two_tile_state():
    """18 x 17 x 17 voxels, 17 * 16 * 16 = 4352 cells: more than one scan tile of 4096, with a sphere whose surface crosses cells on
    both sides of the tile border, so that a triangle count carries across tiles."""
    dims, s = (18, 17, 17), 0.125
    origin = tuple(-0.5 * n * s for n in dims)
    total, count = to.sphere_state(dims, s, origin, (0.02, 0.01, 0.03), 0.93)
    return total, count, None, origin, s


# ---- the stream case ------------------------------------------------------------------------------------------------------------------
STREAM_MAX_TRIANGLES = 4096

# The op list is empty on purpose, as for the plane sweep (the comment in tests/plane_sweep_cases.py): tests/test_stream_cases_host.py
# requires every op a case names to be in ops.FUNCTIONAL_OPS / INPLACE_OPS, two tuples that an earlier schema guard pins, and the ops
# of these calls are listed in ops.FUSION_OPS.  The calls below still go through them, and their outputs are compared.
@stream_cases.case(["sfm_tsdf_integrate", "sfm_tsdf_extract_mesh"], [])
def tsdf_fusion(dev):
    """Three depth maps of 24 x 32 fused into the 23 x 18 x 22 volume and its mesh, two scenes of equal shapes, other poses, depths
    and images: the C entry points on the test's state, outputs and workspace (the state zeroed by a fill on the call's stream
    first), and the functional ops on the same inputs."""
    import torch

    from structure_from_motion_amd import ops

    i = stream_cases.Inst(dev)
    # three spare streams of torch's pool beside this case: four in all, so that every later side stream of
    # tests/test_gpu_streams.py keeps its hardware queue (the comment in tests/register_views_cases.py)
    i.keep_alignment = [torch.cuda.Stream() for _ in range(3)]
    V, H, W, T = 3, 24, 32, STREAM_MAX_TRIANGLES
    a, b = sweep_cases.scene(H, W, V, seed=31, step_deg=4.0), sweep_cases.scene(H, W, V, seed=32, step_deg=7.0)
    nx, ny, nz = PLANE_DIMS
    ox, oy, oz = PLANE_ORIGIN
    other = b["depth"] * 1.02
    other[:, 5:12, 8:20] = np.nan   # a hole: fewer cells are seen twice, so the totals differ as well
    depth, images = i.inp(a["depth"], other), i.inp(a["images"], b["images"])
    poses, K = i.inp(a["poses"], b["poses"]), i.same(np.ascontiguousarray(a["K"].reshape(9)))
    views = i.same(np.arange(V), torch.int32)
    total, count = i.out("sum", (nz, ny, nx), torch.float64), i.out("count", (nz, ny, nx), torch.int32)
    grey_sum, status = i.out("grey_sum", (nz, ny, nx), torch.int32), i.out("status", (V,), torch.int32)
    vertices, grey = i.out("vertices", (T, 3, 3), torch.float64), i.out("grey", (T, 3), torch.float64)
    found = i.out("total", (1,), torch.int64)
    lib = stream_cases._lib()
    ws = i.work(lib.sfm_tsdf_mesh_workspace_bytes(nx, ny, nz))
    i.constant |= {"status"}   # every view is a view
    op = ops.load()

    def call():
        st = stream_cases._st()
        for state in (total, count, grey_sum):
            state.zero_()   # a fresh volume, on the current stream
        stream_cases._check(lib.sfm_tsdf_integrate(total.data_ptr(), count.data_ptr(), grey_sum.data_ptr(), nx, ny, nz, ox, oy, oz, PLANE_VOXEL,
                                                   PLANE_TRUNCATION, depth.data_ptr(), images.data_ptr(), V, H, W, K.data_ptr(),
                                                   poses.data_ptr(), views.data_ptr(), V, status.data_ptr(), st), "sfm_tsdf_integrate")
        stream_cases._check(lib.sfm_tsdf_extract_mesh(total.data_ptr(), count.data_ptr(), grey_sum.data_ptr(), nx, ny, nz, ox, oy, oz,
                                                      PLANE_VOXEL, 2, T, vertices.data_ptr(), grey.data_ptr(), found.data_ptr(),
                                                      ws.data_ptr(), ws.numel(), st), "sfm_tsdf_extract_mesh")
        fresh = (torch.zeros_like(total), torch.zeros_like(count), torch.zeros_like(grey_sum))
        fused = op.tsdf_integrate(*fresh, depth, images, K, poses, views, ox, oy, oz, PLANE_VOXEL, PLANE_TRUNCATION)
        mesh = op.tsdf_extract_mesh(fused[0], fused[1], fused[2], ox, oy, oz, PLANE_VOXEL, 2, T)
        return stream_cases.Returned(fused[:3] + mesh)   # (the statuses are the same in both scenes)
    i.call = call
    return i
