"""Depth maps fused into a surface: a truncated-signed-distance (TSDF) volume that all depth maps are averaged into, and the
triangle mesh of its zero level set by marching tetrahedra (csrc/sfm_tsdf.hip).

Both device results are defined as a fixed sequence of float64 operations (tests/tsdf_oracle.py is the same sequence in NumPy): a
call is reproducible bit for bit, and how the views are split into ``integrate`` calls never changes a result.  ``Mesh.weld``,
``save_ply``, ``volume_bounds`` and ``suggest_voxel_size`` are NumPy only."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from .depth_maps import FilteredDepthMaps, _camera, _integer, _poses


@dataclass
class Mesh:
    """Triangles on the host.  ``vertices`` (T, 3, 3): triangle, corner, coordinate, the normal ``(B - A) x (C - A)`` pointing into
    free space (towards the cameras); ``grey`` (T, 3) or None: the interpolated grey value of every corner."""
    vertices: np.ndarray
    grey: Optional[np.ndarray] = None

    def weld(self):
        """-> (points (M, 3), faces (T, 3) int32, grey (M,) or None): corners that are equal as bytes become one point, in the
        order of their first appearance.  Neighbouring cells compute a shared corner with the same bits, so this closes the mesh."""
        flat = np.ascontiguousarray(np.asarray(self.vertices, dtype=np.float64).reshape(-1, 3))
        if len(flat) == 0:
            return np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int32), (None if self.grey is None else np.zeros(0))
        keys = flat.view(np.dtype((np.void, 24))).reshape(-1)
        _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
        order = np.argsort(first, kind="stable")          # the sorted unique keys in the order of their first appearance
        rank = np.empty(len(order), dtype=np.int64)
        rank[order] = np.arange(len(order))
        faces = rank[inverse.reshape(-1)].reshape(-1, 3).astype(np.int32)
        at = first[order]
        grey = None if self.grey is None else np.asarray(self.grey, dtype=np.float64).reshape(-1)[at]
        return flat[at], faces, grey


def save_ply(path, mesh: Mesh) -> None:
    """The welded mesh as a binary little-endian PLY file: double x, y, z per point (and uchar red, green, blue, the rounded grey,
    with a grey mesh), then ``uchar 3, int32 x 3`` per face."""
    if not isinstance(mesh, Mesh):
        raise ValueError(f"save_ply needs a Mesh, got {type(mesh).__name__}")
    points, faces, grey = mesh.weld()
    fields = [("x", "<f8"), ("y", "<f8"), ("z", "<f8")]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(points)}", "property double x", "property double y",
              "property double z"]
    if grey is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    header += [f"element face {len(faces)}", "property list uchar int vertex_indices", "end_header"]
    vertex = np.zeros(len(points), dtype=fields)
    vertex["x"], vertex["y"], vertex["z"] = points[:, 0], points[:, 1], points[:, 2]
    if grey is not None:
        level = np.clip(np.rint(np.nan_to_num(grey)), 0, 255).astype(np.uint8)
        vertex["red"] = vertex["green"] = vertex["blue"] = level
    face = np.zeros(len(faces), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    face["n"], face["v"] = 3, faces
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(vertex.tobytes())
        f.write(face.tobytes())


def _positive(value, name: str) -> float:
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name} must be a number, got {value!r}")
    value = float(value)
    if not (np.isfinite(value) and value > 0.0):
        raise ValueError(f"{name} must be finite and > 0, got {value!r}")
    return value


def _points_of(points) -> np.ndarray:
    points = np.asarray(points.points if isinstance(points, FilteredDepthMaps) else points, dtype=np.float64)
    if points.ndim < 1 or points.shape[-1] != 3:
        raise ValueError(f"points must have a last dimension of 3, got shape {points.shape}")
    points = points.reshape(-1, 3)
    return points[np.all(np.isfinite(points), axis=1)]


def volume_bounds(points, margin: float = 0.0):
    """-> (low (3,), high (3,)): the box of the finite points (a ``FilteredDepthMaps`` or an array (..., 3)), ``margin`` wider on
    every side."""
    margin = float(margin)
    if not (np.isfinite(margin) and margin >= 0.0):
        raise ValueError(f"margin must be finite and >= 0, got {margin!r}")
    points = _points_of(points)
    if len(points) == 0:
        raise ValueError("volume_bounds needs at least one finite point")
    return points.min(axis=0) - margin, points.max(axis=0) + margin


def suggest_voxel_size(filtered: FilteredDepthMaps, K, pixels: float = 2.0) -> float:
    """``pixels`` times the footprint of a pixel at the median kept depth: ``pixels * median(depth) / K[0, 0]``."""
    if not isinstance(filtered, FilteredDepthMaps):
        raise ValueError(f"suggest_voxel_size needs a FilteredDepthMaps, got {type(filtered).__name__}")
    K = _camera(K)
    pixels = _positive(pixels, "pixels")
    kept = filtered.depth[np.isfinite(filtered.depth)]
    if len(kept) == 0:
        raise ValueError("suggest_voxel_size needs at least one kept depth")
    return pixels * float(np.median(kept)) / abs(float(K[0, 0]))


class TsdfVolume:
    """A volume of ``dims = (nx, ny, nz)`` voxels of ``voxel_size`` whose corner is ``origin``; its state (the sum of the truncated
    distances, the number of views and, ``with_grey``, the sum of the grey values per voxel) lives on the device.  ``truncation``:
    the distance at which a view stops contributing behind a surface (default: four voxels).  A volume above ``max_voxels``
    is refused with ``ValueError`` before any device work (28 bytes a voxel with grey)."""

    def __init__(self, origin, voxel_size: float, dims, truncation: Optional[float] = None, with_grey: bool = False,
                 max_voxels: int = 2**27):
        origin = np.asarray(origin, dtype=np.float64)
        if origin.shape != (3,) or not np.all(np.isfinite(origin)):
            raise ValueError(f"origin must be three finite numbers, got {origin!r}")
        voxel_size = _positive(voxel_size, "voxel_size")
        dims = np.asarray(dims)
        if dims.shape != (3,) or not np.issubdtype(dims.dtype, np.integer) or dims.min() < 1:
            raise ValueError(f"dims must be three integers >= 1 (nx, ny, nz), got {dims!r}")
        max_voxels = _integer(max_voxels, "max_voxels", 1)
        voxels = int(dims[0]) * int(dims[1]) * int(dims[2])
        if voxels > max_voxels or voxels >= 2**31:
            raise ValueError(f"a volume of {voxels} voxels exceeds max_voxels = {max_voxels} (or 2^31 - 1): choose larger voxels")
        truncation = 4.0 * voxel_size if truncation is None else _positive(truncation, "truncation")
        if not isinstance(with_grey, (bool, np.bool_)):
            raise ValueError(f"with_grey must be a bool, got {with_grey!r}")
        self.origin, self.voxel_size, self.truncation = tuple(float(o) for o in origin), voxel_size, truncation
        self.dims, self.with_grey = tuple(int(d) for d in dims), bool(with_grey)
        import torch

        from .. import device

        dev = device.require_gpu()
        shape = self.dims[::-1]
        self.sum = torch.zeros(shape, dtype=torch.float64, device=dev)
        self.count = torch.zeros(shape, dtype=torch.int32, device=dev)
        self.grey_sum = torch.zeros(shape, dtype=torch.int32, device=dev) if with_grey else None

    def state(self):
        return self.sum, self.count, self.grey_sum

    def integrate(self, depth, K, poses, views=None, images=None) -> None:
        """Add the depth maps of ``views`` (default: all, in order) to the volume.  ``depth``: (V, H, W) z-depths, NaN (or
        anything not finite and positive) for no depth; ``K``, ``poses`` (V, 12) as for ``compute_depth_maps``; ``images``: (V, H, W)
        uint8, needed exactly when the volume was made ``with_grey``.  Every argument is checked before any device work
        (``ValueError``), a view index outside the maps among them."""
        depth = np.asarray(depth, dtype=np.float64)
        if depth.ndim != 3 or min(depth.shape) < 1 or depth.shape[1] * depth.shape[2] >= 2**31:
            raise ValueError(f"depth must be a non-empty (V, H, W) array of fewer than 2^31 pixels a view, got shape {depth.shape}")
        V = depth.shape[0]
        K = _camera(K)
        poses = _poses(poses, V)
        views = np.arange(V) if views is None else np.asarray(views)
        if views.ndim != 1 or (views.size and not np.issubdtype(views.dtype, np.integer)):
            raise ValueError(f"views must be a list of view indices, got shape {views.shape} and dtype {views.dtype}")
        if views.size and (views.min() < 0 or views.max() >= V):
            raise ValueError(f"views must index the depth maps 0 .. {V - 1}")
        if (images is not None) != self.with_grey:
            raise ValueError("images are needed exactly when the volume was made with_grey")
        if images is not None:
            images = np.asarray(images)
            if images.dtype != np.uint8 or images.shape != depth.shape:
                raise ValueError(f"images must be a uint8 array of shape {depth.shape}, got {images.dtype} {images.shape}")
        if views.size == 0:
            return
        import torch

        from .. import device

        status = torch.empty((len(views),), dtype=torch.int32, device=self.sum.device)
        device.tsdf_integrate(self.state(), device.to_device(np.ascontiguousarray(depth)),
                              None if images is None else device.to_device(images, torch.uint8), device.to_device(K.reshape(9)),
                              device.to_device(poses), device.to_device(views.astype(np.int32), torch.int32), self.origin, self.voxel_size,
                              self.truncation, status=status)
        if np.any(device.read_tsdf_status(status) != device.TSDF_OK):
            raise RuntimeError("TsdfVolume.integrate: the device refused a view index (SFM_TSDF_BAD_VIEW)")

    def extract_mesh(self, min_count: int = 1) -> Mesh:
        """The zero level set over the cells whose eight voxels were seen by at least ``min_count`` views.  Two device calls: the
        first learns the number of triangles, the second writes them."""
        min_count = _integer(min_count, "min_count", 1, 2**31 - 1)
        if min(self.dims) < 2:
            raise ValueError(f"a mesh needs at least two voxels each way, the volume has {self.dims}")
        from .. import device

        _, _, total = device.tsdf_extract_mesh(self.state(), self.origin, self.voxel_size, min_count, 0)
        found = int(total.cpu().numpy()[0])
        vertices, grey, _ = device.tsdf_extract_mesh(self.state(), self.origin, self.voxel_size, min_count, found)
        return Mesh(vertices.cpu().numpy(), None if grey is None else grey.cpu().numpy())

    def to_host(self):
        """-> (sum (nz, ny, nx) float64, count int32, grey_sum int32 or None) (synchronises)."""
        return (self.sum.cpu().numpy(), self.count.cpu().numpy(), None if self.grey_sum is None else self.grey_sum.cpu().numpy())


def fuse_depth_maps(filtered: FilteredDepthMaps, K, poses, voxel_size: float, truncation: Optional[float] = None, min_count: int = 2,
                    bounds=None) -> Mesh:
    """The filtered depth maps of ``filter_depth_maps`` as one surface: a volume over ``bounds`` = (low, high) (default: the box
    of the kept points, a truncation wider), every map averaged into it with its grey values, and the mesh over the cells that at
    least ``min_count`` views saw.  ``poses``: (V, 12) of all views; the maps are those of ``filtered.refs``.  Every argument is
    checked before any device work (``ValueError``)."""
    if not isinstance(filtered, FilteredDepthMaps):
        raise ValueError(f"fuse_depth_maps needs a FilteredDepthMaps, got {type(filtered).__name__}")
    depth = np.asarray(filtered.depth, dtype=np.float64)
    refs = np.asarray(filtered.refs)
    images = np.asarray(filtered.images)
    if depth.ndim != 3 or len(refs) != len(depth) or images.ndim != 3 or images.shape[1:] != depth.shape[1:]:
        raise ValueError("filtered must hold one (H, W) depth map per entry of refs and images of the same size")
    if refs.size and (refs.min() < 0 or refs.max() >= len(images)):
        raise ValueError("filtered.refs must index filtered.images")
    K = _camera(K)
    poses = _poses(poses, len(images))
    voxel_size = _positive(voxel_size, "voxel_size")
    truncation = 4.0 * voxel_size if truncation is None else _positive(truncation, "truncation")
    min_count = _integer(min_count, "min_count", 1, 2**31 - 1)
    if bounds is None:
        low, high = volume_bounds(filtered, truncation)
    else:
        low, high = (np.asarray(b, dtype=np.float64) for b in bounds)
        if low.shape != (3,) or high.shape != (3,) or not np.all(np.isfinite(low)) or not np.all(np.isfinite(high)) or np.any(high <= low):
            raise ValueError("bounds must be (low, high), two finite triples with low < high")
    dims = np.maximum(np.ceil((high - low) / voxel_size).astype(np.int64), 2)
    volume = TsdfVolume(low, voxel_size, dims, truncation, with_grey=True)
    volume.integrate(depth, K, poses[refs], images=np.ascontiguousarray(images[refs]))
    return volume.extract_mesh(min_count)
