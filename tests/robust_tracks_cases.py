"""Fixtures and the stream case of the outlier-robust triangulation of tracks (sfm_triangulate_tracks_robust, DESIGN.md
section 6ae).

``parity_scene()`` is the input of the parity tests: 8 cameras and 130 points (two full waves and a ragged third), track
lengths 2 .. 12 mixed in one call (beyond 8 a camera is seen twice), 15 % of the pixels shifted by up to +-100 px, in a
random observation order.  ``oracle_run(options)`` is the definition on it, forward and with every track's rows reversed,
computed once per option set and shared.  ``value_scene()`` is the scene of the feature's value condition.

Importing this module registers the stream case of the new entry point in ``stream_cases.CASES``; the two test files of the
feature import it at their top and sort before test_gpu_streams.py and test_stream_cases_host.py, so both of those see the
complete table in a run of the whole suite."""
import functools

import numpy as np

import robust_tracks_oracle as ro
import stream_cases
from structure_from_motion_amd import synthetic

CAMERAS, POINTS = 8, 130
LENGTHS = tuple(range(2, 13))
MAX_ERROR = 9.0                      # px^2
SHIFTED, SHIFT_PX, NOISE_PX = 0.15, 100.0, 0.5
ONE_DEGREE = float(np.radians(1.0))
# (max_hypotheses, min_views, min_angle, refine_steps): both values of each, every pair of values of two options together
# at least once.  Tracks of 7 or more observations (21 pairs) sample ranks at 16 hypotheses; 12-long ones (66) also at 64.
PARITY_OPTIONS = ((16, 2, 0.0, 0), (64, 2, 0.0, 10), (16, 3, ONE_DEGREE, 10), (64, 3, ONE_DEGREE, 0), (16, 2, ONE_DEGREE, 10),
                  (64, 3, 0.0, 0), (16, 3, 0.0, 10), (64, 2, ONE_DEGREE, 0))
MIN_CLEAR = 0.99

# The largest difference between two runs of the definition on the parity scene, rows of every track in run order and
# reversed, over the clear points both runs give an estimate, over the PARITY_OPTIONS with the same refine_steps
# (test_robust_tracks_host.py re-measures it): the absolute difference of the points and of the angles (radians), the
# difference of the errors relative to max(e, 1 px^2).  The device is allowed ten times as much.  Measured without LM:
# points 1.98e-13, angle 4.03e-14, error 1.10e-12; with 10 LM steps, which end at the step limit on some tracks and so
# keep what the two starts differ by: points 1.06e-8, angle 9.44e-11, error 1.06e-7; rounded up.
SPREAD = {0: dict(points=2.5e-13, angle=5e-14, error=1.5e-12), 10: dict(points=1.5e-8, angle=1.2e-10, error=1.5e-7)}
DEVICE_TOLERANCE = {steps: {k: 10.0 * v for k, v in spread.items()} for steps, spread in SPREAD.items()}


def project(K, poses, X, cam):
    R = poses[cam, :9].reshape(-1, 3, 3)
    xc = np.einsum("mij,mj->mi", R, X) + poses[cam, 9:]
    uvw = xc @ K.T
    return uvw[:, :2] / uvw[:, 2:3]


def mixed_tracks(cameras, points, lengths, seed, shifted=SHIFTED, shift_px=SHIFT_PX, noise_px=NOISE_PX):
    """dict(K, poses (C, 12), camera_indices, point_indices int32 (M,), pixels (M, 2), shifted (M,) bool, points_true): point p
    has lengths[p % len(lengths)] observations, in distinct cameras up to ``cameras`` of them and in every camera plus repeats
    beyond; Gaussian pixel noise, a share of the pixels shifted by uniform +-shift_px, the observations in random order."""
    base = synthetic.bundle_problem(cameras, points, per_point=2, seed=seed)
    K, poses, X = base["K"], base["poses_true"], base["points_true"]
    rng = np.random.default_rng(seed + 1000)
    cam, pt = [], []
    for p in range(points):
        k = lengths[p % len(lengths)]
        own = list(rng.permutation(cameras)[:min(k, cameras)]) + list(rng.integers(0, cameras, max(0, k - cameras)))
        cam += own
        pt += [p] * k
    cam, pt = np.array(cam, dtype=np.int32), np.array(pt, dtype=np.int32)
    order = rng.permutation(len(cam))
    cam, pt = cam[order], pt[order]
    pixels = project(K, poses, X[pt], cam) + rng.normal(0.0, noise_px, (len(cam), 2))
    bad = rng.random(len(cam)) < shifted
    pixels[bad] += rng.uniform(-shift_px, shift_px, (int(bad.sum()), 2))
    for a in (cam, pt, pixels, bad):
        a.setflags(write=False)
    return dict(K=K, poses=poses, camera_indices=cam, point_indices=pt, pixels=pixels, shifted=bad, points_true=X)


@functools.lru_cache(maxsize=None)
def parity_scene():
    return mixed_tracks(CAMERAS, POINTS, LENGTHS, seed=3)


@functools.lru_cache(maxsize=None)
def oracle_run(options, reverse=False):
    """The definition on the parity scene for options = (max_hypotheses, min_views, min_angle, refine_steps).  Computed once,
    shared by every test, never changed."""
    max_hypotheses, min_views, min_angle, refine_steps = options
    sc = parity_scene()
    return ro.triangulate(sc["K"], sc["poses"], sc["camera_indices"], sc["point_indices"], sc["pixels"], POINTS, MAX_ERROR,
                          min_views, min_angle, refine_steps, max_hypotheses, reverse=reverse)


def spread_between(a, b, scene_points, point_index):
    """The differences SPREAD names between two results (dicts of the oracle's keys), over the points that are clear in
    ``a`` and have an estimate in both, and over the observations of those points."""
    both = a["clear"][:scene_points] & np.isin(a["status"], (ro.OK, ro.SMALL_ANGLE)) & np.isin(b["status"], (ro.OK, ro.SMALL_ANGLE))
    out = dict(points=0.0, angle=0.0, error=0.0)
    if both.any():
        out["points"] = float(np.abs(a["points"][both] - b["points"][both]).max())
        out["angle"] = float(np.abs(a["angle"][both] - b["angle"][both]).max())
        obs = both[point_index]
        ea, eb = a["obs_error"][obs], b["obs_error"][obs]
        finite = np.isfinite(ea) & np.isfinite(eb)
        assert np.array_equal(np.isfinite(ea), np.isfinite(eb))
        out["error"] = float((np.abs(ea[finite] - eb[finite]) / np.maximum(ea[finite], 1.0)).max())
    return out


@functools.lru_cache(maxsize=None)
def value_scene():
    """``bundle_problem(8, 300, per_point=6, seed=0)`` at its true poses with 15 % of the pixels shifted by up to +-100 px."""
    base = synthetic.bundle_problem(8, 300, per_point=6, seed=0)
    problem, bad = synthetic.corrupt_observations(base, 0.15, 100.0, seed=1)
    return dict(K=problem["K"], poses=problem["poses_true"], camera_indices=problem["camera_indices"],
                point_indices=problem["point_indices"], pixels=problem["pixels"], shifted=bad)


def recovered(inlier, scene, points):
    """(tracks that hold a shifted observation, those of them whose inliers are exactly the clean observations)."""
    pt, bad = scene["point_indices"], scene["shifted"]
    dirty = np.bincount(pt[bad], minlength=points) > 0
    wrong = np.bincount(pt[np.asarray(inlier, dtype=bool) == bad], minlength=points) > 0
    return int(dirty.sum()), int(np.count_nonzero(dirty & ~wrong))


# ------------------------------------------------------------------------------------------------------
# every status in one call
# ------------------------------------------------------------------------------------------------------
# cameras without rotation at these centres: a baseline of 1 in x and in y, one of 2, a hair's (4) and a camera close to the
# point (5), whose rows weigh little in a DLT and whose pixel therefore takes nearly all of a disagreement
RIG_CENTRES = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (2.0, 0.0, 0.0), (0.01, 0.0, 0.0), (1.0, 0.0, 4.0))
RIG_POINT = (0.2, -0.3, 5.0)
RIG_BEHIND = (0.3, 0.2, -5.0)


def rig_poses():
    poses = np.zeros((len(RIG_CENTRES), 12))
    poses[:, :9] = np.eye(3).reshape(9)
    poses[:, 9:] = -np.array(RIG_CENTRES)
    return poses


def rig_track(cams, X=RIG_POINT, shifts=None):
    """(cams, pixels): the noise-free pixels of X in the rig's cameras ``cams``, pixel q moved by shifts[q]."""
    cams = np.asarray(cams, dtype=np.int32)
    uv = project(synthetic.BENCH_K, rig_poses(), np.repeat(np.asarray(X, dtype=np.float64)[None], len(cams), axis=0), cams)
    for q, shift in (shifts or {}).items():
        uv[q] += shift
    return cams, uv


def _rig_run(cams, uv, **options):
    return ro.triangulate(synthetic.BENCH_K, rig_poses(), cams, np.zeros(len(cams), dtype=np.int64), uv, 1, MAX_ERROR, **options)


@functools.lru_cache(maxsize=None)
def status_scene():
    """One call that holds every status a call without a bad index can give, each set by every step of the definition that can
    set it, among OK tracks: dict(poses, camera_indices, point_indices, pixels, points, min_angle, names (P,), status (P,) and
    step (P,) as constructed).  70 points, two waves; threshold MAX_ERROR, min_views 2.  Each special track:
      few / none      one observation, and none at all: FEW_VIEWS;
      one_camera      three observations of one camera: DEGENERATE (step 0);
      twice           cameras 0, 2, 2, 1: the same-camera pair is skipped, OK with every flag;
      behind          the pixels of a point behind cameras 0 and 1: their only hypothesis fails the depth test, NO_CONSENSUS (3);
      behind_mixed    those two pixels followed by three good ones: OK, the two flagged out;
      shifted_pair    two observations, one pixel 40 px off the epipolar line: a hypothesis but no inlier, NO_CONSENSUS (3);
      one_camera_left the close camera 5 with its pixel 20 px off, then camera 0 twice: the DLT of (5, 0) leaves nearly all of
                      the 20 px to camera 5, the winner's inliers are the two of camera 0, NO_CONSENSUS (4);
      refit_loses     the same with an offset that keeps camera 5 within the threshold at the winner (its pair's DLT) and
                      puts it beyond at the refit (two rows of camera 0 against it): inliers of one camera, NO_CONSENSUS (5);
      narrow          camera 0 and three observations of camera 4, two of them 1 px further along the baseline: the winner is
                      the wider pair, the refit over all four is narrower; min_angle lies between the two: SMALL_ANGLE (5)."""
    base, wide = rig_track([0, 4, 4, 4]), rig_track([0, 4, 4, 4], shifts={2: (-1.0, 0.0), 3: (-1.0, 0.0)})
    flat = _rig_run(*wide)
    d = tracks_rays(wide[0][[0, 2]], wide[1][[0, 2]])
    min_angle = 0.5 * (float(flat["angle"][0]) + d)
    assert float(_rig_run(*base)["angle"][0]) < float(flat["angle"][0]) < min_angle < d
    # the offset of refit_loses: the middle of the range in which camera 5 is within the threshold at the winner and beyond
    # it at the refit (found on a grid of 0.005 px)
    def lost_at_the_refit(x):
        r = _rig_run(*rig_track([5, 0, 0], shifts={0: (0.0, float(x))}))
        return r["status"][0] == ro.NO_CONSENSUS and r["step"][0] == 5
    inside = [x for x in np.arange(4.5, 5.5, 0.005) if lost_at_the_refit(x)]
    assert len(inside) >= 10
    offset = float(inside[len(inside) // 2])
    special = {
        3: ("few", rig_track([1]), ro.FEW_VIEWS, 0),
        9: ("one_camera", rig_track([3, 3, 3], shifts={1: (0.5, 0.0)}), ro.DEGENERATE, 0),
        14: ("twice", rig_track([0, 2, 2, 1]), ro.OK, 5),
        20: ("behind", rig_track([0, 1], RIG_BEHIND), ro.NO_CONSENSUS, 3),
        27: ("behind_mixed", (np.array([0, 1, 2, 3, 0], dtype=np.int32),
                              np.vstack([rig_track([0, 1], RIG_BEHIND)[1], rig_track([2, 3, 0])[1]])), ro.OK, 5),
        33: ("shifted_pair", rig_track([0, 1], shifts={1: (0.0, 40.0)}), ro.NO_CONSENSUS, 3),
        41: ("one_camera_left", rig_track([5, 0, 0], shifts={0: (0.0, 20.0)}), ro.NO_CONSENSUS, 4),
        48: ("refit_loses", rig_track([5, 0, 0], shifts={0: (0.0, offset)}), ro.NO_CONSENSUS, 5),
        55: ("narrow", wide, ro.SMALL_ANGLE, 5),
        66: ("none", (np.zeros(0, dtype=np.int32), np.zeros((0, 2))), ro.FEW_VIEWS, 0),
    }
    P = 70
    rng = np.random.default_rng(11)
    cam, pt, uv, names, status, step = [], [], [], [], [], []
    for p in range(P):
        if p in special:
            name, (c, q), st, sp = special[p]
        else:
            X = np.array(RIG_POINT) + rng.uniform(-0.3, 0.3, 3)
            c, q = rig_track([0, 1, 2, 3][:2 + p % 3], X)
            q = q + rng.normal(0.0, NOISE_PX, q.shape)
            name, st, sp = "ok", ro.OK, 5
        cam.append(c), pt.append(np.full(len(c), p, dtype=np.int32)), uv.append(q)
        names.append(name), status.append(st), step.append(sp)
    cam, pt, uv = np.concatenate(cam), np.concatenate(pt), np.vstack(uv)
    # a track's own order numbers its hypotheses, so it stays; the tracks are shuffled among each other: observation m of the
    # call is the next unused observation of the track that a random permutation puts at m
    nxt = {p: list(np.nonzero(pt == p)[0]) for p in range(P)}
    src = np.array([nxt[int(p)].pop(0) for p in pt[rng.permutation(len(cam))]], dtype=np.int64)
    cam2, pt2, uv2 = cam[src], pt[src], uv[src]
    return dict(poses=rig_poses(), camera_indices=cam2, point_indices=pt2, pixels=uv2, points=P, min_angle=min_angle,
                names=names, status=np.array(status, dtype=np.uint8), step=np.array(step))


def tracks_rays(cams, uv):
    """The angle between the two rays of the two-view DLT point of two rig observations."""
    import tracks_oracle as to

    poses = rig_poses()
    X = to.triangulate_pair_dlt(synthetic.BENCH_K, poses[cams[0]], poses[cams[1]], uv[0], uv[1])
    d = to.rays(poses[cams, :9].reshape(1, 2, 3, 3), poses[cams, 9:][None], X[None])[0]
    return float(np.arccos(min(1.0, d[0] @ d[1])))


# ------------------------------------------------------------------------------------------------------
# the stream case
# ------------------------------------------------------------------------------------------------------
@stream_cases.case(["sfm_triangulate_tracks_robust"], [])
def triangulate_tracks_robust(dev):
    """2 000 points with tracks of 2 .. 12 observations, 16 hypotheses (tracks of 7 and more sample ranks), a 1 degree angle
    limit and 10 LM steps, through ``device.triangulate_tracks_robust`` on the test's buffers and workspace: two scenes of equal
    shapes whose pixels differ."""
    import torch

    from structure_from_motion_amd import device

    i = stream_cases.Inst(dev)
    P = 2000
    a, b = mixed_tracks(CAMERAS, P, LENGTHS, seed=21), mixed_tracks(CAMERAS, P, LENGTHS, seed=22)
    M = len(a["pixels"])
    assert M == len(b["pixels"])
    poses = i.inp(a["poses"], b["poses"])
    cam, pt = i.inp(a["camera_indices"], b["camera_indices"]), i.inp(a["point_indices"], b["point_indices"])
    pix = i.inp(a["pixels"], b["pixels"])
    out = (i.out("points", (P, 3), torch.float64), i.out("status", (P,), torch.uint8), i.out("obs_error", (M,), torch.float64),
           i.out("inlier", (M,), torch.uint8), i.out("angle", (P,), torch.float64), i.out("info", (6,), torch.int64))
    ws = i.work(stream_cases._lib().sfm_tracks_robust_workspace_bytes(P, M))
    K = a["K"]

    def call():
        _, used = device.triangulate_tracks_robust(poses, cam, pt, pix, P, K, MAX_ERROR, 2, ONE_DEGREE, 10, 16, out=out,
                                                   workspace=ws)
        assert used is ws
    i.call = call
    return i
