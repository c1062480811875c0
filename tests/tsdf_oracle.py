"""The NumPy definition of TSDF fusion and of marching-tetrahedra extraction, written from the definition and not
from csrc/sfm_tsdf.hip.  Every step is an elementwise float64 ``+ - * /`` in the order the definition states, so the device result
is compared with it as bytes.  Vectorised over the voxels of a volume and over the cells of one (tetrahedron, sign pattern);
explicit loops over views, tetrahedra and patterns."""
import numpy as np

from plane_sweep_oracle import camera_matrices, dot3, project, same_bytes   # noqa: F401  (same_bytes is for the tests)

OK, BAD_VIEW = 0, 1

# the six tetrahedra of the Kuhn split about the diagonal 0-7; corner q of a cell is (i + (q & 1), j + ((q >> 1) & 1), k + ((q >> 2) & 1))
TETRAHEDRA = ((0, 1, 3, 7), (0, 3, 2, 7), (0, 2, 6, 7), (0, 6, 4, 7), (0, 4, 5, 7), (0, 5, 1, 7))


def centres(dims, origin, voxel_size):
    """(cx [nx], cy [ny], cz [nz]): ``o + (i + 0.5) s`` per axis."""
    s = np.float64(voxel_size)
    return tuple(np.float64(o) + (np.arange(n, dtype=np.float64) + 0.5) * s for n, o in zip(dims, origin))


def integrate(state, depth, images, K, poses, views, origin, voxel_size, truncation):
    """``state``: (sum f64 [nz, ny, nx], count int32, grey_sum int32 or None), left unchanged.  -> (sum, count, grey_sum, status)."""
    total, count, grey_sum = (None if a is None else np.array(a) for a in state)
    nz, ny, nx = total.shape
    depth = np.asarray(depth, dtype=np.float64)
    V, H, W = depth.shape
    poses = np.asarray(poses, dtype=np.float64).reshape(V, 12)
    views = np.asarray(views).reshape(-1)
    status = np.zeros(len(views), dtype=np.int32)
    assert (images is None) == (grey_sum is None)
    cx, cy, cz = centres((nx, ny, nz), origin, voxel_size)
    X = [np.broadcast_to(cx[None, None, :], (nz, ny, nx)), np.broadcast_to(cy[None, :, None], (nz, ny, nx)),
         np.broadcast_to(cz[:, None, None], (nz, ny, nx))]
    Km, _ = camera_matrices(K)
    trunc = np.float64(truncation)
    for n, v in enumerate(int(v) for v in views):
        if not 0 <= v < V:
            status[n] = BAD_VIEW
            continue
        with np.errstate(all="ignore"):
            u, w, z = project(Km, poses[v], X)
            x, y = np.floor(u + 0.5), np.floor(w + 0.5)
            ok = (z > 0.0) & (x >= 0.0) & (x < float(W)) & (y >= 0.0) & (y < float(H))
            xi, yi = np.where(ok, x, 0.0).astype(np.int64), np.where(ok, y, 0.0).astype(np.int64)
            d = depth[v][yi, xi]
            ok &= np.isfinite(d) & (d > 0.0)
            sdf = d - z
            ok &= ~(sdf < -trunc)
            f = np.where(sdf < trunc, sdf / trunc, 1.0)
        total = np.where(ok, total + np.where(ok, f, 0.0), total)
        count = np.where(ok, count + 1, count).astype(np.int32)
        if grey_sum is not None:
            grey_sum = np.where(ok, grey_sum + images[v][yi, xi].astype(np.int32), grey_sum).astype(np.int32)
    return total, count, grey_sum, status


def _edge(lo, hi, f, g, P):
    """The vertex on the edge of two corners (lists of per-cell arrays), ``lo`` the one of the lower linear voxel index."""
    with np.errstate(all="ignore"):
        t = f[lo] / (f[lo] - f[hi])
        point = [P[lo][a] + t * (P[hi][a] - P[lo][a]) for a in range(3)]
        grey = None if g is None else g[lo] + t * (g[hi] - g[lo])
    return point, grey


def extract_mesh(total, count, grey_sum, origin, voxel_size, min_count=1, max_triangles=None):
    """-> (vertices [T, 3, 3], grey [T, 3] or None, total triangles): T = max_triangles, or the true count when that is None; rows
    beyond the true count are NaN."""
    total, count = np.asarray(total, dtype=np.float64), np.asarray(count, dtype=np.int32)
    nz, ny, nx = total.shape
    cx, cy, cz = centres((nx, ny, nz), origin, voxel_size)
    k, j, i = (a.reshape(-1) for a in np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij"))
    with np.errstate(all="ignore"):
        value = total / count.astype(np.float64)
        shade = None if grey_sum is None else np.asarray(grey_sum).astype(np.float64) / count.astype(np.float64)
    bits = [((q & 1), (q >> 1) & 1, (q >> 2) & 1) for q in range(8)]
    f = [value[k + b[2], j + b[1], i + b[0]] for b in bits]
    g = None if shade is None else [shade[k + b[2], j + b[1], i + b[0]] for b in bits]
    P = [(cx[i + b[0]], cy[j + b[1]], cz[k + b[2]]) for b in bits]
    valid = np.ones(len(i), dtype=bool)
    for b in bits:
        valid &= count[k + b[2], j + b[1], i + b[0]] >= min_count
    negative = [fq < 0 for fq in f]
    cell = np.arange(len(i))
    keys, points, greys = [], [], []
    for t, tet in enumerate(TETRAHEDRA):
        for pattern in range(1, 15):
            neg = [q for m, q in enumerate(tet) if (pattern >> m) & 1]
            pos = [q for m, q in enumerate(tet) if not (pattern >> m) & 1]
            at = valid.copy()
            for m, q in enumerate(tet):
                at &= negative[q] if (pattern >> m) & 1 else ~negative[q]
            if not at.any():
                continue
            if len(neg) == 1:
                (a,), (b, c, d) = neg, pos
                triangles = [((a, b), (a, c), (a, d))]
            elif len(neg) == 3:
                (a,), (b, c, d) = pos, neg
                triangles = [((a, b), (a, c), (a, d))]
            else:
                (a, b), (c, d) = neg, pos
                triangles = [((a, c), (a, d), (b, d)), ((a, c), (b, d), (b, c))]
            D = [np.float64(len(neg) * sum(bits[q][a] for q in pos) - len(pos) * sum(bits[q][a] for q in neg)) for a in range(3)]
            fa = [fq[at] for fq in f]
            ga = None if g is None else [gq[at] for gq in g]
            Pa = [[c[at] for c in Pq] for Pq in P]
            for order, triangle in enumerate(triangles):
                corners = [_edge(min(p, q), max(p, q), fa, ga, Pa) for p, q in triangle]
                A, B, C = (c[0] for c in corners)
                with np.errstate(all="ignore"):
                    e, h = [B[a] - A[a] for a in range(3)], [C[a] - A[a] for a in range(3)]
                    n = [e[1] * h[2] - e[2] * h[1], e[2] * h[0] - e[0] * h[2], e[0] * h[1] - e[1] * h[0]]
                    swap = dot3(n[0], D[0], n[1], D[1], n[2], D[2]) < 0.0
                vertex = np.stack([np.stack(A, -1), np.where(swap[:, None], np.stack(C, -1), np.stack(B, -1)),
                                   np.where(swap[:, None], np.stack(B, -1), np.stack(C, -1))], axis=1)
                keys.append(cell[at] * 12 + t * 2 + order)
                points.append(vertex)
                if g is not None:
                    ga_, gb_, gc_ = (c[1] for c in corners)
                    greys.append(np.stack([ga_, np.where(swap, gc_, gb_), np.where(swap, gb_, gc_)], axis=1))
    found = sum(len(q) for q in keys)
    rows = found if max_triangles is None else int(max_triangles)
    vertices = np.full((rows, 3, 3), np.nan)
    grey = None if grey_sum is None else np.full((rows, 3), np.nan)
    if found:
        order = np.argsort(np.concatenate(keys), kind="stable")[:rows]
        vertices[:len(order)] = np.concatenate(points)[order]
        if grey is not None:
            grey[:len(order)] = np.concatenate(greys)[order]
    return vertices, grey, found


def sphere_state(dims=(12, 12, 12), voxel_size=0.25, origin=(-1.5, -1.5, -1.5), centre=(0.03, -0.02, 0.05), radius=0.9173):
    """The analytic signed distance to a sphere (negative inside), ``count`` 1 everywhere: -> (sum, count)."""
    cx, cy, cz = centres(dims, origin, voxel_size)
    r = np.sqrt((cx[None, None, :] - centre[0]) ** 2 + (cy[None, :, None] - centre[1]) ** 2 + (cz[:, None, None] - centre[2]) ** 2)
    return r - radius, np.ones(r.shape, dtype=np.int32)
