"""Directed inputs for the triangulation of multi-view tracks (csrc/sfm_tracks.hip): one track per status
and per broken rule, neighbours that send a wave down the Jacobi route, every ``min_views``, tracks of up to 300
observations, tracks of one camera and non-finite input.  Imported by tests/test_tracks_cases_host.py, which checks on
the CPU that the oracle alone meets each case's preconditions, and by tests/test_gpu_tracks_cases.py, which runs the same
cases on the device; a plain helper module like geometry_cases.py.

A case is a dict: poses (C, 12), cam, pt (M,), uv (M, 2), P, min_views, min_angle (radians), max_error (px^2), and
- ``expect``: {point: status} the construction promises;
- ``directed``: points built to sit on one side of a threshold, which keep MARGIN (relative) from it;
- ``loose``: points whose status rounding decides (only the co-centred pairs of case 5).
Every other point keeps more than STATUS_BAND from both thresholds (``threshold_gap``), so that the device has to give
the oracle's status exactly."""
import numpy as np

import geometry_cases as gc
import tracks_oracle as to
from structure_from_motion_amd import synthetic

K = synthetic.BENCH_K
MIN_ANGLE = np.radians(1.0)
MAX_ERROR = 16.0
MARGIN = 1e-3
REFINES = (0, 10)
IDENTITY = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])


def make(poses, cam, pt, uv, P, min_views=2, min_angle=MIN_ANGLE, max_error=MAX_ERROR, **notes):
    case = dict(poses=np.asarray(poses, dtype=np.float64), cam=np.asarray(cam, dtype=np.int32), pt=np.asarray(pt, dtype=np.int32),
                uv=np.asarray(uv, dtype=np.float64).reshape(-1, 2), P=int(P), min_views=min_views, min_angle=min_angle,
                max_error=max_error, expect={}, directed=[], loose=[])
    case.update(notes)
    return case


def oracle(case, refine, **override):
    kw = dict(min_views=case["min_views"], min_angle=case["min_angle"], max_error=case["max_error"], refine_steps=refine)
    kw.update(override)
    return to.triangulate(K, case["poses"], case["cam"], case["pt"], case["uv"], case["P"], **kw)


def largest_error(case, out):
    """The largest finite-or-inf obs_error of each point (NaN where it has none)."""
    max_e = np.full(case["P"], np.nan)
    has = ~np.isnan(out["obs_error"])
    np.fmax.at(max_e, case["pt"][has], out["obs_error"][has])
    return max_e


def threshold_gap(case, out):
    """(P,) the relative distance of each point's angle and largest error from the case's thresholds, the smaller of the
    two; inf where the point has neither, or the threshold is 0 or inf."""
    gap = np.full(case["P"], np.inf)
    with np.errstate(invalid="ignore"):
        if case["min_angle"] > 0.0:
            gap = np.fmin(gap, np.abs(out["angle"] - case["min_angle"]) / case["min_angle"])
        if np.isfinite(case["max_error"]) and case["max_error"] > 0.0:
            gap = np.fmin(gap, np.abs(largest_error(case, out) - case["max_error"]) / case["max_error"])
    return gap


def depth_gap(case, out):
    """(P,) the smallest |depth| of a point in a camera of its own, relative to its distance from that camera: the
    cheirality test's own threshold is 0.  inf where the point is not finite."""
    X = out["points"][case["pt"]]
    pose = case["poses"][case["cam"]]
    R = pose[:, :9].reshape(-1, 3, 3)
    c = np.einsum("mij,mj->mi", R, X) + pose[:, 9:]
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(c[:, 2]) / np.linalg.norm(c, axis=1)
    gap = np.full(case["P"], np.inf)
    np.fmin.at(gap, case["pt"], np.where(np.isfinite(rel), rel, np.inf))
    return gap


def project(pose, X):
    return gc.project(K, np.asarray(pose)[None], np.asarray(X, dtype=np.float64)[None])[0]


def ring_cameras(n, seed, radius=0.6):
    """n cameras with their centres on a circle of ``radius`` about the Z axis (any two at least 2 radius sin(pi / n)
    apart: 4 degrees and more seen from z = 4 .. 6 at n = 8), turned by up to 3 degrees about X and Y."""
    rng = np.random.default_rng(seed)
    poses = np.zeros((n, 12))
    for i in range(n):
        a = 2.0 * np.pi * i / n
        R = synthetic.rotation_xy(rng.uniform(-3.0, 3.0), rng.uniform(-3.0, 3.0))
        centre = np.array([radius * np.cos(a), radius * np.sin(a), rng.uniform(-0.1, 0.1)])
        poses[i] = np.concatenate([R.reshape(9), -R @ centre])
    return poses


def random_tracks(poses, lengths, seed, noise_px=0.5, cameras=None, shuffle=True):
    """Point i (uniform in x, y in [-0.5, 0.5], z in [4, 6]) seen by lengths[i] distinct cameras of ``cameras`` (default:
    all of poses), with Gaussian pixel noise: (cam, pt, uv, points); the observations in random order."""
    rng = np.random.default_rng(seed)
    cameras = np.arange(len(poses)) if cameras is None else np.asarray(cameras)
    n = len(lengths)
    X = np.column_stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n), rng.uniform(4.0, 6.0, n)])
    cam = np.concatenate([rng.permutation(cameras)[:k] for k in lengths] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    pt = np.repeat(np.arange(n), lengths)
    uv = gc.project(K, poses[cam], X[pt]) + rng.normal(0.0, noise_px, (len(cam), 2))
    if shuffle:
        order = rng.permutation(len(cam))
        cam, pt, uv = cam[order], pt[order], uv[order]
    return cam, pt, uv, X


# ---- 1. every status, and several broken rules at once ---------------------------------------------------------------
def every_status():
    """One constructed track per status (points 0 .. 6, the construction test_tracks_host.py had, at its max_error of
    4 px^2), then 7: behind + small angle + large error, 8: small angle + large error, and 9: no observation at all, past
    the last observed index."""
    poses = np.array([IDENTITY,
                      np.concatenate([synthetic.rotation_xy(0.0, -5.0).reshape(9), [0.5, 0.0, 0.0]]),
                      np.concatenate([synthetic.rotation_xy(0.0, 5.0).reshape(9), [-0.5, 0.0, 0.0]]),
                      np.concatenate([np.eye(3).reshape(9), [0.5, 0.0, 0.0]])])
    X = np.array([0.2, -0.1, 5.0])
    cam, pt, uv = [], [], []

    def add(p, c, pix):
        cam.append(c)
        pt.append(p)
        uv.append(pix)

    def see(c, Y):
        return project(poses[c], Y)

    add(0, 0, see(0, X)), add(0, 1, see(1, X)), add(0, 2, see(2, X))               # 0 OK
    add(1, 0, see(0, X))                                                              # 1 FEW_VIEWS
    add(2, 0, K[:2, 2]), add(2, 3, K[:2, 2])                # 2 DEGENERATE: parallel rays, the point at infinity
    behind = np.array([0.2, -0.1, -5.0])
    add(3, 0, see(0, behind)), add(3, 1, see(1, behind))                            # 3 BEHIND
    far = np.array([0.2, -0.1, 400.0])
    add(4, 0, see(0, far)), add(4, 1, see(1, far))                                  # 4 SMALL_ANGLE
    add(5, 0, see(0, X)), add(5, 1, see(1, X) + [15.0, 0.0]), add(5, 2, see(2, X))   # 5 LARGE_ERROR
    # 6 has no observation: FEW_VIEWS
    # a 15 px shift across the epipolar line (the baseline is along x) leaves the depth and costs (7.5 px)^2 per view
    far_behind = np.array([0.2, -0.1, -400.0])
    add(7, 0, see(0, far_behind)), add(7, 1, see(1, far_behind) + [0.0, 15.0])      # 7 BEHIND, also narrow and off
    add(8, 0, see(0, far)), add(8, 1, see(1, far) + [0.0, 15.0])                    # 8 SMALL_ANGLE, also off
    # 9 has no observation and lies past the last observed index: FEW_VIEWS
    expect = {0: to.OK, 1: to.FEW_VIEWS, 2: to.DEGENERATE, 3: to.BEHIND, 4: to.SMALL_ANGLE, 5: to.LARGE_ERROR,
              6: to.FEW_VIEWS, 7: to.BEHIND, 8: to.SMALL_ANGLE, 9: to.FEW_VIEWS}
    return make(poses, cam, pt, uv, 10, max_error=4.0, expect=expect, directed=[0, 3, 4, 5, 7, 8])


def tiled(case, copies):
    """``copies`` copies of every track of the case, copy r of point p at r P + p: cyclic, so that a wave of 64 holds
    every kind."""
    P, M = case["P"], len(case["cam"])
    shift = np.repeat(np.arange(copies) * P, M)
    out = dict(case, cam=np.tile(case["cam"], copies), pt=(np.tile(case["pt"], copies) + shift).astype(np.int32),
               uv=np.tile(case["uv"], (copies, 1)), P=P * copies)
    out["expect"] = {r * P + p: s for r in range(copies) for p, s in case["expect"].items()}
    out["directed"] = [r * P + p for r in range(copies) for p in case["directed"]]
    out["loose"] = [r * P + p for r in range(copies) for p in case["loose"]]
    out["period"] = P
    return out


# ---- 2. neighbour independence ---------------------------------------------------------------------------------------
FILLERS = ("few", "nan", "parallel", "outlier")
TWIN_SHIFT = 8.7e-4   # two parallel cameras this far apart see z = 5 under 0.01 degrees


def _neighbour_poses():
    """Cameras 0 .. 7 on a ring, and 8 .. 15 their twins: the same rotation, the centre TWIN_SHIFT further along x."""
    ring = ring_cameras(8, 41)
    twins = ring.copy()
    for i in range(8):
        R = ring[i, :9].reshape(3, 3)
        twins[i, 9:] = ring[i, 9:] - R @ np.array([TWIN_SHIFT, 0.0, 0.0])
    return np.vstack([ring, twins])


def neighbours_alone():
    """64 noisy (0.5 px) well-conditioned tracks of lengths 2 .. 6 on the ring cameras."""
    poses = _neighbour_poses()
    cam, pt, uv, _ = random_tracks(poses, 2 + np.arange(64) % 5, 42, cameras=np.arange(8))
    return make(poses, cam, pt, uv, 64)


def _filler(kind):
    poses = _neighbour_poses()
    rng = np.random.default_rng(43)
    if kind == "few":      # one observation each
        cam, pt, uv, _ = random_tracks(poses, np.ones(64, dtype=np.int64), 44, cameras=np.arange(8))
    elif kind == "nan":    # a good track with one NaN coordinate
        cam, pt, uv, _ = random_tracks(poses, 2 + np.arange(64) % 5, 45, cameras=np.arange(8))
        first = np.array([np.nonzero(pt == p)[0][p % 2] for p in range(64)])
        uv[first, np.arange(64) % 2] = np.nan
    elif kind == "parallel":   # a camera and its twin: a disparity of 0.26 px under 0.5 px of noise
        ring = rng.integers(0, 8, 64)
        cam = np.column_stack([ring, ring + 8]).reshape(-1)
        pt = np.repeat(np.arange(64), 2)
        X = np.column_stack([rng.uniform(-0.5, 0.5, 64), rng.uniform(-0.5, 0.5, 64), rng.uniform(4.0, 6.0, 64)])
        uv = gc.project(K, poses[cam], X[pt]) + rng.normal(0.0, 0.5, (128, 2))
    elif kind == "outlier":    # a good track of 3 .. 6 views with one pixel 60 px off
        cam, pt, uv, _ = random_tracks(poses, 3 + np.arange(64) % 4, 46, cameras=np.arange(8))
        first = np.array([np.nonzero(pt == p)[0][0] for p in range(64)])
        uv[first] += np.where(np.arange(64)[:, None] % 2 == 0, [60.0, 0.0], [0.0, -60.0])
    else:
        raise KeyError(kind)
    return make(poses, cam, pt, uv, 64)


def neighbours_mixed(kind):
    """The 64 tracks of neighbours_alone at the even points and 64 fillers of one kind at the odd ones: every wave is
    mixed, and each point's own observations keep their order."""
    a, b = neighbours_alone(), _filler(kind)
    return make(a["poses"], np.concatenate([a["cam"], b["cam"]]), np.concatenate([2 * a["pt"], 2 * b["pt"] + 1]),
                np.vstack([a["uv"], b["uv"]]), 128, kind=kind)


# ---- 3. min_views ----------------------------------------------------------------------------------------------------
MIN_VIEWS = (2, 3, 4, 7)


def view_counts():
    """400 points on 8 ring cameras: point i < 380 has 1 + i % 8 observations, the last 20 none."""
    lengths = np.concatenate([1 + np.arange(380) % 8, np.zeros(20, dtype=np.int64)])
    poses = ring_cameras(8, 51)
    cam, pt, uv, _ = random_tracks(poses, lengths, 52)
    return make(poses, cam, pt, uv, 400, lengths=lengths)


# ---- 4. long tracks --------------------------------------------------------------------------------------------------
LONG_LENGTHS = (7, 63, 64, 65, 300, 300, 65)
LONG_CYCLE, LONG_OUTLIER = 5, 6   # the points whose track cycles over 3 cameras / carries one 15 px outlier


def long_tracks():
    """300 random cameras (centres in a disc of radius 1, turned by up to 5 / 10 degrees) and tracks of 7, 63, 64, 65 and
    300 distinct cameras, one of 300 observations that cycles over 3 cameras and one of 65 with a single pixel 15 px off;
    0.5 px noise.  Each point's observations come in random order, the points' runs interleaved."""
    rng = np.random.default_rng(61)
    poses = np.zeros((300, 12))
    for i in range(300):
        R = synthetic.rotation_xy(rng.uniform(-5.0, 5.0), rng.uniform(-10.0, 10.0))
        r, a = np.sqrt(rng.random()), rng.uniform(0.0, 2.0 * np.pi)
        poses[i] = np.concatenate([R.reshape(9), -R @ np.array([r * np.cos(a), r * np.sin(a), rng.uniform(-0.2, 0.2)])])
    n = len(LONG_LENGTHS)
    X = np.column_stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n), rng.uniform(4.0, 6.0, n)])
    cams = [rng.permutation(300)[:k] for k in LONG_LENGTHS]
    cams[LONG_CYCLE] = np.tile(rng.permutation(300)[:3], 100)
    cam = np.concatenate(cams)
    pt = np.repeat(np.arange(n), LONG_LENGTHS)
    uv = gc.project(K, poses[cam], X[pt]) + rng.normal(0.0, 0.5, (len(cam), 2))
    uv[np.nonzero(pt == LONG_OUTLIER)[0][40]] += [9.0, -12.0]
    order = rng.permutation(len(cam))
    return make(poses, cam[order], pt[order], uv[order], n)


def reversed_rows(case):
    """The case with each point's observations in the opposite order (the oracle's own sensitivity to the row order)."""
    return dict(case, cam=case["cam"][::-1].copy(), pt=case["pt"][::-1].copy(), uv=case["uv"][::-1].copy())


# ---- 5. tracks of one camera -----------------------------------------------------------------------------------------
ONE_CAMERA_POSES = np.array([
    IDENTITY,
    np.concatenate([synthetic.rotation_xy(4.0, -7.0).reshape(9), [0.4, -0.1, 0.2]]),
    np.concatenate([gc.rotation((1.0, 2.0, 3.0), 25.0).reshape(9), [-0.3, 0.25, 0.1]]),
])
CO_CENTRED_SPLIT = 40.0   # px between the two pixels of a co-centred pair


def one_camera(thresholds):
    """``thresholds``: "default" (min_angle 0, max_error inf) or "app" (1 degree, 16 px^2).  Cameras 0 .. 2: the identity
    and two general poses; 3: camera 1 again under another index; 4: camera 1's centre under another rotation.
    Points 0 .. 35: tracks of 2 .. 5 observations that all name one camera, the pixels equal, 3 px apart and 40 px apart
    (observation j at the first pixel + j times the step): DEGENERATE.  36: the control, two observations from camera 0
    and one from camera 1 of one point: OK.  37, 38: pairs of distinct cameras with one centre (1 and 3, 1 and 4) whose
    pixels point CO_CENTRED_SPLIT px apart: never OK under the app thresholds, whichever way the rounding goes."""
    R1 = ONE_CAMERA_POSES[1, :9].reshape(3, 3)
    centre = -R1.T @ ONE_CAMERA_POSES[1, 9:]
    R4 = gc.rotation((0.0, 1.0, 0.0), 3.0) @ R1
    poses = np.vstack([ONE_CAMERA_POSES, ONE_CAMERA_POSES[1], np.concatenate([R4.reshape(9), -R4 @ centre])])
    X = np.array([0.3, -0.2, 5.0])
    cam, pt, uv, expect = [], [], [], {}
    p = 0
    for c in range(3):
        for step in (0.0, 3.0, 40.0):
            for n in (2, 3, 4, 5):
                for j in range(n):
                    cam.append(c), pt.append(p), uv.append(project(poses[c], X) + [j * step, 0.0])
                expect[p] = to.DEGENERATE
                p += 1
    for c, off in ((0, [0.0, 0.0]), (0, [0.5, -0.5]), (1, [0.2, 0.3])):
        cam.append(c), pt.append(p), uv.append(project(poses[c], X) + off)
    expect[p] = to.OK
    control = p
    loose = []
    for other in (3, 4):
        p += 1
        cam.extend([1, other]), pt.extend([p, p])
        uv.extend([project(poses[1], X), project(poses[other], X) + [0.0, CO_CENTRED_SPLIT]])
        loose.append(p)
    kw = dict(min_angle=0.0, max_error=np.inf) if thresholds == "default" else {}
    return make(poses, cam, pt, uv, p + 1, expect=expect, directed=[control], loose=loose, control=control, **kw)


def check_co_centred(case, out):
    """Not OK; where an estimate was written, its largest error is above the app threshold by the margin."""
    max_e = largest_error(case, out)
    for p in case["loose"]:
        assert out["status"][p] != to.OK, p
        if out["status"][p] != to.DEGENERATE:
            assert max_e[p] > MAX_ERROR * (1.0 + MARGIN), (p, max_e[p])# ---- 6. non-finite input ---------------------------------------------------------------------------------------------
def non_finite():
    """160 noisy tracks of lengths 2 .. 6 on 8 ring cameras, and camera 8 = camera 3 with a NaN entry.  Every 16th point
    from 3 has a NaN pixel coordinate, from 7 an infinite one (+inf and -inf, u and v by turns), and from 11 an observation
    moved to camera 8: ``touched`` lists them; the 64-lane waves hold 12 of them each among 52 others."""
    poses = np.vstack([ring_cameras(8, 71), ring_cameras(8, 71)[3]])
    poses[8, 4] = np.nan
    cam, pt, uv, _ = random_tracks(poses, 2 + np.arange(160) % 5, 72, cameras=np.arange(8))
    touched = []
    for i, p in enumerate(range(3, 160, 16)):
        uv[np.nonzero(pt == p)[0][i % 2], i % 2] = np.nan
        touched.append(p)
    for i, p in enumerate(range(7, 160, 16)):
        uv[np.nonzero(pt == p)[0][-1], i % 2] = np.inf if i % 4 < 2 else -np.inf
        touched.append(p)
    for i, p in enumerate(range(11, 160, 16)):
        cam[np.nonzero(pt == p)[0][i % 2]] = 8
        touched.append(p)
    return make(poses, cam, pt, uv, 160, touched=sorted(touched), expect={p: to.DEGENERATE for p in touched})


# ---- every case by name ----------------------------------------------------------------------------------------------
def _with_min_views(min_views):
    return lambda: dict(view_counts(), min_views=min_views)


CASES = {"every_status": every_status, "every_status_tiled": lambda: tiled(every_status(), 19),
         "neighbours_alone": neighbours_alone}
CASES.update({f"neighbours_{kind}": (lambda kind=kind: neighbours_mixed(kind)) for kind in FILLERS})
CASES.update({f"min_views_{m}": _with_min_views(m) for m in MIN_VIEWS})
CASES.update({"long_tracks": long_tracks, "one_camera_default": lambda: one_camera("default"),
              "one_camera_app": lambda: one_camera("app"), "non_finite": non_finite})
