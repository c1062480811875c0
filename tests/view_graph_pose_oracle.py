"""The NumPy definition of the pose entry of the view-graph call (csrc/sfm_view_graph_pose.hip): the four poses
of ``oracle.sfm_oracle.recover_all_r_t``, the cheirality vote of ``cheirality_pass`` over every inlier (no item skipped), the
angle between the two viewing rays and its lower median; the motions of the tests, the points a scene was made from, and the
margins of the cheirality tests that the exact vote comparison rests on.  Imported by tests/test_view_graph_pose_host.py and
tests/test_gpu_view_graph_pose.py."""
import numpy as np

import homography_oracle as ho
from oracle import sfm_oracle as orc

OK, NO_MODEL, NOT_ESSENTIAL, NO_VOTE, BAD_OFFSETS = range(5)
STATUS = ("ok", "no_model", "not_essential", "no_vote", "bad_offsets")
DISTANCE = 50.0
POSE_BYTES = 128

# bench's rotation with a twentieth of its baseline: the true parallax is about 0.025 / 5 rad = 0.29 degrees against 5.7 for bench
MOTIONS = dict(ho.MOTIONS)
MOTIONS["bench_narrow"] = (ho.MOTIONS["bench"][0], ho.MOTIONS["bench"][1] * 0.05, False)
# a general rotation with a baseline (gen12 itself has none)
MOTIONS["gen12_t"] = (ho.MOTIONS["gen12"][0], np.array([0.3, -0.1, 0.05]), False)


def motion_scene(name, n, seed, noise_px=0.0, outlier_fraction=0.0):
    R, t, planar = MOTIONS[name]
    return ho.scene(R, t, planar, n, seed, noise_px, outlier_fraction)


def scene_points(name, n, seed):
    """The points ``motion_scene(name, n, seed, ...)`` projects, in the frame of view 1: the first draws of its generator."""
    rng = np.random.default_rng(seed)
    X = np.empty((n, 3))
    X[:, 0] = rng.uniform(-1.0, 1.0, n)
    X[:, 1] = rng.uniform(-1.0, 1.0, n)
    z = rng.uniform(4.0, 6.0, n)
    X[:, 2] = 5.0 + 0.2 * X[:, 0] - 0.1 * X[:, 1] if MOTIONS[name][2] else z
    return X


def true_parallax(X, R, t):
    """The angle at each point between the directions to the two camera centres (0 and -R^T t), by the arc cosine."""
    to_b = X + R.T @ t
    c = np.sum(X * to_b, axis=1) / (np.linalg.norm(X, axis=1) * np.linalg.norm(to_b, axis=1))
    return np.arccos(np.clip(c, -1.0, 1.0))


def essential(R, t):
    """[t]x R of a unit t."""
    t = t / np.linalg.norm(t)
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]]) @ R


def candidates(E):
    """(4, 12) rows R (9) | t (3) in the entry's order (R1, t), (R1, -t), (R2, t), (R2, -t) from ``recover_all_r_t``."""
    R1, R2, t1 = orc.recover_all_r_t(np.asarray(E, dtype=np.float64).reshape(3, 3))
    return np.array([np.concatenate([R.reshape(9), t]) for R in (R1, R2) for t in (t1, -t1)])


def vote(corr, poses, distance_threshold=DISTANCE):
    """(pass (4, n) bool, votes (4,), best): every item counts; best is the first maximum, -1 when all votes are zero."""
    passes = np.array([orc.cheirality_pass(corr, p[:9].reshape(3, 3), p[9:], distance_threshold) for p in poses]).reshape(4, -1)
    votes = passes.sum(axis=1).astype(np.int64)
    best = int(np.argmax(votes)) if votes.any() else -1
    return passes, votes, best


def ray_angles(corr, R):
    """The angle between a = (xa, ya, 1) and c = R^T (xb, yb, 1), in the operation order of the entry."""
    xa, ya, xb, yb = corr[:, 0], corr[:, 1], corr[:, 2], corr[:, 3]
    a = (xa, ya, np.ones_like(xa))
    c = [(R[0, j] * xb + R[1, j] * yb) + R[2, j] * 1.0 for j in range(3)]
    w0 = a[1] * c[2] - a[2] * c[1]
    w1 = a[2] * c[0] - a[0] * c[2]
    w2 = a[0] * c[1] - a[1] * c[0]
    n = np.sqrt((w0 * w0 + w1 * w1) + w2 * w2)
    d = (a[0] * c[0] + a[1] * c[1]) + a[2] * c[2]
    return np.arctan2(n, d)


def lower_median(angles):
    return np.sort(angles)[(len(angles) - 1) // 2]


def pair_pose(corr, e_mask, E, distance_threshold=DISTANCE, poses=None):
    """The record of one pair: dict(status, R, t, votes, best, median_angle, angles (n,), NaN off the passing inliers).  ``E``
    None: no model.  ``poses``: the (4, 12) candidates to vote on instead of ``candidates(E)`` (a device's own)."""
    n = len(corr)
    out = dict(status=NO_MODEL, R=np.full((3, 3), np.nan), t=np.full(3, np.nan), votes=np.zeros(4, np.int64), best=-1,
               median_angle=np.nan, angles=np.full(n, np.nan))
    if E is None:
        return out
    if poses is None:
        try:
            poses = candidates(E)
        except orc.OracleDegenerateSample:
            out["status"] = NOT_ESSENTIAL
            return out
    items = np.nonzero(np.asarray(e_mask) != 0)[0]
    passes, votes, best = vote(corr[items], poses, distance_threshold)
    if best < 0:
        out["status"] = NO_VOTE
        return out
    R, t = poses[best][:9].reshape(3, 3), poses[best][9:]
    chosen = items[passes[best]]
    out["angles"][chosen] = ray_angles(corr[chosen], R)
    out.update(status=OK, R=R, t=t, votes=votes, best=best, median_angle=lower_median(out["angles"][chosen]))
    return out


def cheirality_margins(corr, R, t, distance_threshold=DISTANCE):
    """How far the three tests of ``cheirality_pass`` are from their limits over the items: (the least |depth + 1e-8| over both
    depths, the least relative distance of |X| from the threshold).  Under the mirrored pose (R, -t) the depths change sign and
    the norm stays, so one call covers an antipodal pair when the depths are also kept away from +1e-8."""
    if len(corr) == 0:
        return np.inf, np.inf
    P2 = np.eye(4)
    P2[:3, :3], P2[:3, 3] = R, t
    X = orc.triangulate_dlt(corr, np.eye(4), P2)
    z2 = (np.hstack([X, np.ones((len(X), 1))]) @ P2.T)[:, 2]
    depths = np.concatenate([X[:, 2], z2])
    depth_margin = min(np.min(np.abs(depths + orc.CHEIRALITY_TOLERANCE)), np.min(np.abs(depths - orc.CHEIRALITY_TOLERANCE)))
    norm = np.sqrt((X * X).sum(axis=1))
    return float(depth_margin), float(np.min(np.abs(norm - distance_threshold) / distance_threshold))


def decode(pose_bytes):
    """A (Q, 128) uint8 pose table as a list of dicts in ``pair_pose``'s keys (without the angles)."""
    dt = np.dtype([("R", "<f8", (3, 3)), ("t", "<f8", (3,)), ("median_angle", "<f8"), ("votes", "<i4", (4,)), ("best", "<i4"),
                   ("status", "<i4")])
    assert dt.itemsize == POSE_BYTES
    table = np.ascontiguousarray(pose_bytes).reshape(-1).view(dt)
    return [dict(status=int(r["status"]), R=r["R"].copy(), t=r["t"].copy(), votes=r["votes"].astype(np.int64), best=int(r["best"]),
                 median_angle=float(r["median_angle"])) for r in table]


KIND_CASES = (("pan10", 400), ("plane_bench", 350), ("bench_narrow", 400), ("bench", 250), ("gen12", 90))
KIND_SEED = 7


def kind_scenes():
    """The scenes of the kinds-and-seed test: 0.5 px noise, 30 % outliers."""
    return [motion_scene(name, n, KIND_SEED, 0.5, 0.3) for name, n in KIND_CASES]


EDGE_COUNTS = (1, 2, 3, 256, 257, 1025)   # k passing items: the smallest, and both sides of one and of four block strides


def edge_case_fixture():
    """The pairs of the selection test, all of one noise-free ``bench`` motion so that every unmasked item passes under the
    true pose: (corr (N, 4), offset (Q + 1,), e_mask (N,), R, t).  Pairs 0-5: k = EDGE_COUNTS items, all unmasked; 6: 257 unmasked
    items interleaved with 257 masked ones; 7: one item 600 times (all keys equal); 8: two items interleaved 300 + 301 times (the
    rank falls on the boundary between the two runs of equal keys); 9: one item with xa moved by 0 .. 299 ulps (angles that
    differ in the lowest digit of their bit patterns)."""
    sc = motion_scene("bench", 2200, 17)
    base, parts, masks, at = sc["corr"], [], [], 0
    for k in EDGE_COUNTS:
        parts.append(base[at:at + k])
        masks.append(np.where(np.arange(k) % 5 == 0, 2, 1))
        at += k
    parts.append(base[at:at + 514])
    masks.append(np.arange(514) % 2)
    at += 514
    parts.append(np.repeat(base[at:at + 1], 600, axis=0))
    masks.append(np.ones(600, np.int64))
    two = np.empty((601, 4))
    two[0::2], two[1::2] = base[at + 2], base[at + 1]
    parts.append(two)
    masks.append(np.ones(601, np.int64))
    ulps = np.repeat(base[at + 3:at + 4], 300, axis=0)
    ulps[:, 0] += np.arange(300) * np.spacing(ulps[0, 0])
    parts.append(ulps)
    masks.append(np.ones(300, np.int64))
    offset = np.zeros(len(parts) + 1, dtype=np.int64)
    offset[1:] = np.cumsum([len(p) for p in parts])
    return np.ascontiguousarray(np.concatenate(parts)), offset, np.concatenate(masks).astype(np.uint8), sc["R"], sc["t"]
