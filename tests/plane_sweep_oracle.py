"""The NumPy definition of plane-sweep depth maps and of their consistency filter, written from the definition and
not from csrc/sfm_plane_sweep.hip.  Every step is an elementwise float64 ``+ - * / sqrt`` in the order the definition states, so
the device result is compared with it as bytes.  Vectorised over the pixels of a view; explicit loops over window rows and
columns, sources and depths.  No ``np.sum`` over a window: its pairwise order is not the definition's.

Every 3-term product sum is ``(a0*b0 + a1*b1) + a2*b2`` (``dot3``)."""
import numpy as np

OK, BAD_REFERENCE = 0, 1


def dot3(a0, b0, a1, b1, a2, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def mul3(A, B):
    return [[dot3(A[i][0], B[0][j], A[i][1], B[1][j], A[i][2], B[2][j]) for j in range(3)] for i in range(3)]


def camera_matrices(K):
    """K rebuilt from its five entries, and its inverse in closed form (nested lists of float64)."""
    K = np.asarray(K, dtype=np.float64).reshape(9)
    fx, sk, cx, fy, cy = K[0], K[1], K[2], K[4], K[5]
    zero, one = np.float64(0.0), np.float64(1.0)
    ff = fx * fy
    Km = [[fx, sk, cx], [zero, fy, cy], [zero, zero, one]]
    Ki = [[one / fx, -sk / ff, (sk * cy - cx * fy) / ff], [zero, one / fy, -cy / fy], [zero, zero, one]]
    return Km, Ki


def split_pose(pose):
    """A pose row, R row-major (9) then t (3), as ((3, 3), (3,))."""
    pose = np.asarray(pose, dtype=np.float64).reshape(12)
    return pose[:9].reshape(3, 3), pose[9:]


def homography(K, pose_r, pose_s, z):
    """G = K (Rrel + trel e3^T / z) K^-1 of a reference pose, a source pose and a depth."""
    (Rr, tr), (Rs, ts) = split_pose(pose_r), split_pose(pose_s)
    M = [[dot3(Rs[a, 0], Rr[b, 0], Rs[a, 1], Rr[b, 1], Rs[a, 2], Rr[b, 2]) for b in range(3)] for a in range(3)]
    trel = [ts[a] - dot3(M[a][0], tr[0], M[a][1], tr[1], M[a][2], tr[2]) for a in range(3)]
    for a in range(3):
        M[a][2] = M[a][2] + trel[a] / np.float64(z)
    Km, Ki = camera_matrices(K)
    return np.array(mul3(mul3(Km, M), Ki), dtype=np.float64)


def present(src, ref, views):
    return 0 <= src < views and src != ref


def warp(image, G):
    """The bilinear sample of ``image`` (uint8 [H, W]) at G (x, y, 1) for every integer pixel (x, y); NaN where invalid."""
    H, W = image.shape
    img = image.astype(np.float64)
    x, y = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        X = (G[0, 0] * x + G[0, 1] * y) + G[0, 2]
        Y = (G[1, 0] * x + G[1, 1] * y) + G[1, 2]
        Wd = (G[2, 0] * x + G[2, 1] * y) + G[2, 2]
        ok = Wd > 0.0
        inv = 1.0 / Wd
        u, v = X * inv, Y * inv
        ok &= (u >= 0.0) & (u < float(W - 1)) & (v >= 0.0) & (v < float(H - 1))
        xf, yf = np.where(ok, np.floor(u), 0.0), np.where(ok, np.floor(v), 0.0)
        fx, fy = u - xf, v - yf
        x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
        p00, p10, p01, p11 = img[y0, x0], img[y0, x0 + 1], img[y0 + 1, x0], img[y0 + 1, x0 + 1]
        top = p00 + fx * (p10 - p00)
        bot = p01 + fx * (p11 - p01)
        b = top + fy * (bot - top)
    return np.where(ok, b, np.nan)


def window_sums(q, radius):
    """Σ q over the (2 radius + 1)^2 window of every pixel: each row left to right first, then the row sums top to bottom; NaN
    where the window leaves the image."""
    H, W = q.shape
    w = 2 * radius + 1
    out = np.full((H, W), np.nan)
    if H < w or W < w:
        return out
    with np.errstate(all="ignore"):
        rows = q[:, 0:W - w + 1].copy()
        for dx in range(1, w):
            rows = rows + q[:, dx:W - w + 1 + dx]
        total = rows[0:H - w + 1].copy()
        for dy in range(1, w):
            total = total + rows[dy:H - w + 1 + dy]
    out[radius:H - radius, radius:W - radius] = total
    return out


def scores(a, sa, va, b, radius, min_variance):
    """1 - NCC of the reference grey values ``a`` (with their sums) and the warped samples ``b``; NaN where invalid."""
    n = np.float64((2 * radius + 1) ** 2)
    gate = np.float64(min_variance) * n * n
    with np.errstate(all="ignore"):
        sb, sbb, sab = window_sums(b, radius), window_sums(b * b, radius), window_sums(a * b, radius)
        vb = n * sbb - sb * sb
        num = n * sab - sa * sb
        ok = np.isfinite(va) & np.isfinite(vb) & np.isfinite(num) & (va >= gate) & (vb >= gate)
        c = 1.0 - num / np.sqrt(va * vb)
        ok &= np.isfinite(c)   # va vb == 0 under min_variance == 0
    return np.where(ok, c, np.nan)


def aggregate(costs, top_k, min_sources):
    """The valid scores ([slots, H, W], NaN = invalid) in ascending order, the first min(top_k or all, valid) added in that order,
    over their count; NaN with fewer than min_sources valid."""
    valid = np.isfinite(costs)
    count = valid.sum(axis=0)
    ordered = np.sort(np.where(valid, costs, np.inf), axis=0)
    take = np.minimum(top_k, count) if top_k > 0 else count
    acc = ordered[0].copy()
    with np.errstate(all="ignore"):
        for i in range(1, costs.shape[0]):
            acc = np.where(i < take, acc + ordered[i], acc)
        cost = acc / take.astype(np.float64)
    return np.where((count >= min_sources) & (count >= 1), cost, np.nan)


def winners(values, eligible, z):
    """-> (depth, index int32, cost) [H, W] of one reference from ``values`` [D, H, W] of the hypotheses at the depths ``z`` [D]:
    the eligible hypothesis of lowest value, ties to the lower index (index -1, depth and cost NaN without one), and the parabola
    step in inverse depth: for a winner 0 < i < D - 1 whose neighbours are both eligible and whose
    den = (before - cost) + (after - cost) > 0, with o = 0.5 (before - after) / den and j = i + 1 for o > 0, else i - 1, the depth
    1 / (1 / z_i + |o| (1 / z_j - 1 / z_i)) in place of z_i."""
    D, H, W = values.shape
    value = np.where(eligible, values, np.nan)
    best, best_cost = np.full((H, W), -1, dtype=np.int32), np.full((H, W), np.nan)
    for d in range(D):
        with np.errstate(all="ignore"):
            better = eligible[d] & ((best < 0) | (value[d] < best_cost))
        best[better] = d
        best_cost[better] = value[d][better]
    has = best >= 0
    at = np.where(has, best, 0)
    with np.errstate(all="ignore"):
        zi = z[at]
        depth = np.where(has, zi, np.nan)
        inner = has & (best > 0) & (best < D - 1)
        before = np.take_along_axis(value, np.clip(at - 1, 0, D - 1)[None], axis=0)[0]
        after = np.take_along_axis(value, np.clip(at + 1, 0, D - 1)[None], axis=0)[0]
        den = (before - best_cost) + (after - best_cost)
        take = inner & np.isfinite(before) & np.isfinite(after) & (den > 0.0)
        o = 0.5 * (before - after) / den
        zj = z[np.clip(np.where(o > 0.0, at + 1, at - 1), 0, D - 1)]
        q = 1.0 / zi + np.abs(o) * (1.0 / zj - 1.0 / zi)
        refined = 1.0 / q
    return np.where(take, refined, depth), best, best_cost


def plane_sweep(images, K, poses, refs, sources, depths, radius, top_k=0, min_sources=1, min_variance=1.0):
    """-> dict(depth [R, H, W], index int32, cost, status int32 [R], volume [R, D, H, W])."""
    images = np.asarray(images)
    V, H, W = images.shape
    poses = np.asarray(poses, dtype=np.float64).reshape(V, 12)
    refs, sources = np.asarray(refs).reshape(-1), np.asarray(sources)
    depths = np.asarray(depths, dtype=np.float64)
    R, S, D = len(refs), sources.shape[1], depths.shape[1]
    n = np.float64((2 * radius + 1) ** 2)
    out = dict(depth=np.full((R, H, W), np.nan), index=np.full((R, H, W), -1, dtype=np.int32), cost=np.full((R, H, W), np.nan),
               status=np.zeros(R, dtype=np.int32), volume=np.full((R, D, H, W), np.nan))
    for r in range(R):
        ref = int(refs[r])
        if not 0 <= ref < V:
            out["status"][r] = BAD_REFERENCE
            continue
        a = images[ref].astype(np.float64)
        sa, saa = window_sums(a, radius), window_sums(a * a, radius)
        with np.errstate(all="ignore"):
            va = n * saa - sa * sa
        volume = out["volume"][r]
        for d in range(D):
            z = depths[r, d]
            if not (np.isfinite(z) and z > 0.0):
                continue
            per_source = [scores(a, sa, va, warp(images[int(src)], homography(K, poses[ref], poses[int(src)], z)), radius, min_variance)
                          for src in sources[r] if present(int(src), ref, V)]
            if per_source:
                volume[d] = aggregate(np.stack(per_source), top_k, min_sources)
        out["depth"][r], out["index"][r], out["cost"][r] = winners(volume, np.isfinite(volume), depths[r])
    return out


def back_project(Ki, pose, x, y, d):
    """The world point of pixel (x, y) of a view at depth d: R^T (d K^-1 (x, y, 1) - t)."""
    R, t = split_pose(pose)
    with np.errstate(all="ignore"):
        e = [((Ki[i][0] * x + Ki[i][1] * y) + Ki[i][2]) * d - t[i] for i in range(3)]
        return [dot3(R[0, i], e[0], R[1, i], e[1], R[2, i], e[2]) for i in range(3)]


def project(Km, pose, X):
    """-> (u, v, z) of a world point in a view: Y = R X + t, p = K Y, u = p0 / p2, v = p1 / p2, z = Y2."""
    R, t = split_pose(pose)
    with np.errstate(all="ignore"):
        Y = [dot3(R[i, 0], X[0], R[i, 1], X[1], R[i, 2], X[2]) + t[i] for i in range(3)]
        p = [dot3(Km[i][0], Y[0], Km[i][1], Y[1], Km[i][2], Y[2]) for i in range(3)]
        return p[0] / p[2], p[1] / p[2], Y[2]


def filter_depth_maps(depth, K, poses, refs, sources, max_pixel_error=1.0, max_relative_depth_error=0.01, min_consistent=2):
    """-> dict(count int32 [R, H, W], filtered [R, H, W], points [R, H, W, 3], status int32 [R])."""
    depth = np.asarray(depth, dtype=np.float64)
    V, H, W = depth.shape
    poses = np.asarray(poses, dtype=np.float64).reshape(V, 12)
    refs, sources = np.asarray(refs).reshape(-1), np.asarray(sources)
    R = len(refs)
    Km, Ki = camera_matrices(K)
    out = dict(count=np.zeros((R, H, W), dtype=np.int32), filtered=np.full((R, H, W), np.nan), points=np.full((R, H, W, 3), np.nan),
               status=np.zeros(R, dtype=np.int32))
    x = np.broadcast_to(np.arange(W, dtype=np.float64)[None, :], (H, W))
    y = np.broadcast_to(np.arange(H, dtype=np.float64)[:, None], (H, W))
    limit = np.float64(max_pixel_error) * np.float64(max_pixel_error)
    for r in range(R):
        ref = int(refs[r])
        if not 0 <= ref < V:
            out["status"][r] = BAD_REFERENCE
            continue
        d = depth[ref]
        has = np.isfinite(d)
        Xw = back_project(Ki, poses[ref], x, y, d)
        count = np.zeros((H, W), dtype=np.int32)
        with np.errstate(all="ignore"):
            near = np.float64(max_relative_depth_error) * d
            for src in sources[r]:
                src = int(src)
                if not present(src, ref, V):
                    continue
                u, v, z = project(Km, poses[src], Xw)
                xs, ys = np.floor(u + 0.5), np.floor(v + 0.5)
                ok = has & (z > 0.0) & (xs >= 0.0) & (xs < float(W)) & (ys >= 0.0) & (ys < float(H))
                xi, yi = np.where(ok, xs, 0.0).astype(np.int64), np.where(ok, ys, 0.0).astype(np.int64)
                ds = depth[src][yi, xi]
                ok &= np.isfinite(ds)
                Xb = back_project(Ki, poses[src], np.where(ok, xs, 0.0), np.where(ok, ys, 0.0), ds)
                xr, yr, zr = project(Km, poses[ref], Xb)
                ex, ey = xr - x, yr - y
                ok &= (ex * ex + ey * ey <= limit) & (np.abs(zr - d) <= near)
                count += ok
        keep = has & (count >= min_consistent)
        out["count"][r] = count
        out["filtered"][r] = np.where(keep, d, np.nan)
        out["points"][r] = np.where(keep[..., None], np.stack(Xw, axis=-1), np.nan)
    return out


def same_bytes(a, b):
    """Equal as bytes, a NaN equal to any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)))
