"""Headless incremental structure from motion over N synthetic views: a two-view seed on views 0 and 1
(``estimate_essential_mat_with_ransac`` -> ``recover_r_t_from_e`` -> ``triangulate_tracks``), then view after view
registered by ``estimate_pose_pnp_with_ransac`` against the points triangulated so far, new tracks triangulated from every
registered view that sees them, and ``bundle_adjust`` over the registered cameras (camera 0 fixed) after each view and at
the end.  ``bundle_solver="dense"`` (the default of ``run``) uses the dense solver and takes at most 64 views;
``"auto"`` (the default of the command line) uses the dense solver while at most 64 cameras are registered and the
iterative one above that, and takes up to 1 024 views.  Both give the same result up to 64 views.  The scene is
``synthetic.multi_view_scene``: cameras on an arc ``--step-deg`` (5) degrees apart, tracks of 2 to N observations,
Gaussian pixel noise and a fraction of the observations replaced by random pixels.  Prints the views registered, each
view's rotation error and translation error (in units of |t_1|, the scale of the seed), the RMS reprojection error of the
final bundle adjustment and the points that end OK, as JSON.

``tracks="given"`` (the default) takes the scene's tracks as they are.  ``tracks="matches"`` starts from pairwise matches
instead (``synthetic.pairwise_matches``: views up to three apart, 10 % wrong matches): every pair is verified by the
essential-matrix RANSAC and keeps its winner's inliers (a pair without a model is dropped), ``build_tracks`` turns them into
tracks, and the same reconstruction runs on the built observations.  The output then also holds the build's info and the
fraction of OK tracks whose features all belong to one true point.  ``verify="batched"`` (``--verify batched``) verifies all
pairs in one ``verify_pairs`` call instead of one essential-matrix RANSAC per pair: a homography and a five-point essential
pass per pair, the pairs whose kind is not ``"none"`` kept with the inliers of the model their kind names, and the number of
pairs of each kind added to the output.  ``seed_pair="auto"`` (``--seed-pair auto``, with ``--tracks matches --verify batched``)
starts from the pair ``choose_seed_pair`` picks among the verified pairs, gated on the median triangulation angle of its
inliers (``--seed-min-angle`` degrees), instead of from views 0 and 1: the pair's pose comes from the same ``verify_pairs``
call (``relative_pose=True``), its first view sits at the identity, and the errors are reported in that gauge (the true poses
relative to that view, in units of the pair's true baseline).  The output then also holds ``seed_pair`` and the pair's
``median_angle_deg``.

``rotations="global"`` (``--rotations global``, with ``--tracks matches --verify batched``) also averages the relative rotations
of the verified pairs into one global rotation per view before any point exists (``average_graph_rotations``: Huber at one
degree from the spanning tree, then Cauchy from Huber's result), and adds ``global_rotations`` to the output: each view's
rotation error against the truth in the gauge of the reconstruction's first view, the solver's status and step counts, and the
pairs whose rotation disagrees with the result by more than ``--drop-inconsistent-pairs`` degrees (5 when it is not given).
``--drop-inconsistent-pairs DEG`` also removes those pairs' matches before ``build_tracks``.  Without these flags the output is
what it was.

``positions="global"`` (``--positions global``, with ``--rotations global``) goes on to average the pairs' translation
directions into one position per view (``average_graph_translations`` on the global rotations: Huber at the sine of two
degrees from the spanning tree with the warm-up, then Cauchy from Huber's result), and adds ``global_positions`` to the output:
each view's centre error against the truth after the scale-and-shift alignment in which the rotations are taken as given (in
units of the first pair's true baseline), the solver's status and step counts, and the pairs whose direction disagrees with the
result by more than the residual limit.  ``register="global"`` (``--register global``, with ``--positions global``) starts the
reconstruction from those poses (``global_poses``) instead of from a seed pair and a PnP chain: every track is triangulated
from all registered views at once and the bundle adjustment follows; the per-view errors are reported as for the incremental
route, and ``bundle`` holds the cost of the first adjustment before and after.

``bundle_loss`` (``--bundle-loss``) gives every bundle adjustment a robust loss (``"huber"`` or ``"cauchy"`` with
``bundle_loss_scale`` pixels); the drop rules stay as they are, and ``rms_px`` is then computed from the
squared errors of the adjusted observations, since the adjuster's cost is a sum of rho.

``focal_error`` (``--focal-error 0.05``) runs the whole pipeline with a camera matrix whose focal lengths are that fraction
off, as a guess from image metadata would be.  ``bundle_refine`` (``--bundle-refine focal[,principal_point]``) frees those
intrinsics in the final bundle adjustment (the dense solver, so at most 64 views).  With either, the output
holds ``focal``: the relative focal error before and after, and the camera matrix the run ends with.

``refine_pairs`` (``--refine-pairs K``, with ``--tracks matches --verify batched``) refines every verified pair's relative pose
on its inliers with up to K rounds (``refine_relative_poses``) before the seed pair is chosen and before the
averaging solvers run, so ``global_rotations`` and ``global_positions`` follow from the refined poses.  The output then holds
``pair_refinement``: the median and the largest pairwise rotation and translation-direction error against the scene's truth,
before and after.  0, the default, is the path without it.

``triangulation="robust"`` (``--triangulation robust``) triangulates with ``triangulate_tracks_robust`` (per-track RANSAC,
DESIGN.md §6ae): one call instead of triangulating, dropping the observations above the threshold and triangulating once
more; the observations it flags out on points that got an estimate become inactive.  The output then holds
``triangulation``.  ``plain``, the default, is the path without it.

``register="batched"`` (``--register batched``) registers the views in rounds instead of one at a time: each round hands every
unregistered view with at least 30 observations of OK points to one ``register_views`` call (a P3P RANSAC pass and the
refinement of its winner per view), accepts every view that comes back ``"ok"`` with at least 30 inliers, then
triangulates the pending tracks and adjusts once; the loop ends when a round accepts nothing.  A view's gate is 10 extra inliers or a quarter of its observations,
whichever is more, so a view that sees the model poorly waits for a later round.  A round triangulates long tracks in one go,
which ``triangulation="robust"`` handles far better than the plain repair (profiles/register_views/README.md).  The route is P3P:
``pnp_solver`` left unset means ``"p3p"`` there (``"dlt"`` on the other routes, as before), and ``"dlt"`` is refused.  The
output then holds ``registration_rounds``: the number of rounds and the views accepted in each.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lib.bundle.bundle import bundle_adjust
from lib.common.feature import Feature
from lib.epipolar.eight_point import create_trivial_matches, recover_r_t_from_e
from lib.epipolar.epipolar_ransac import estimate_essential_mat_with_ransac
from lib.epipolar.view_graph import choose_seed_pair, refine_relative_poses, verify_pairs
from lib.feature_matching.matching import Match
from lib.multiview.rotation_averaging import average_graph_rotations, inconsistent_pairs
from lib.multiview.tracks import build_tracks, triangulate_tracks, triangulate_tracks_robust
from lib.multiview.translation_averaging import average_graph_translations, global_poses
from lib.pnp.pnp import estimate_pose_pnp_with_ransac
from lib.pnp.registration import register_views
from structure_from_motion_amd import _native, device, synthetic

DENSE_MAX_VIEWS = 64   # the dense bundle adjuster's camera limit
MAX_VIEWS = 1024       # with bundle_solver="auto": a bound of the app (host-side bookkeeping and run time)
BUNDLE_SOLVERS = ("dense", "auto")
BUNDLE_LOSSES = device.BUNDLE_LOSSES
TRACK_SOURCES = ("given", "matches")
TRIANGULATIONS = ("plain", "robust")
VERIFY_ROUTES = ("loop", "batched")
SEED_PAIRS = ("first", "auto")
ROTATION_ROUTES = ("incremental", "global")
POSITION_ROUTES = ("incremental", "global")
REGISTER_ROUTES = ("incremental", "global", "batched")
# The scene's cameras stand on an arc a few degrees apart, nearly on a line, where directions fix the positions along the line
# only weakly and the alternation of translation averaging converges slowly: on the default 8 views the library's default of 500
# steps leaves view 1 nearer to view 2's true centre than to its own, 3 000 steps per loss do not.
POSITION_STEPS = 3000
INCONSISTENT_DEG = 5.0   # a pair is reported as inconsistent above this residual unless --drop-inconsistent-pairs says otherwise
MIN_PNP_INLIERS = 30
# The gate of the batched route, as a fraction of a view's observations.  RANSAC keeps the lowest-error model among the gated
# ones, and with the sequential route's gate of 10 a pose fitted to 14 of a far view's 1 150 observations beat the true one
# (637 inliers, RMS error 6.3 px^2).  The scene replaces 20 % of the observations, and the true pose of the farthest of 8 views
# still holds 47 % of them against points of the seed pair alone; a model of a few outliers holds about 1 %.  A view below the
# gate is not lost: it waits for the next round, when more points stand.
BATCHED_MIN_EXTRA_FRACTION = 0.25


def _pose(R, t) -> np.ndarray:
    return np.concatenate([np.asarray(R, dtype=np.float64).reshape(9), np.asarray(t, dtype=np.float64).reshape(3)])


def _errors(K, poses, X, cam, pt, uv) -> np.ndarray:
    """Squared reprojection error of each observation (+inf behind the camera)."""
    R = poses[cam, :9].reshape(-1, 3, 3)
    xc = np.einsum("mij,mj->mi", R, X[pt]) + poses[cam, 9:]
    with np.errstate(divide="ignore", invalid="ignore"):
        p = (xc @ K.T)[:, :2] / xc[:, 2:3]
        e = np.sum((p - uv) ** 2, axis=1)
    return np.where(xc[:, 2] > 0, e, np.inf)


class Reconstruction:
    """The incremental state: a pose per registered view, a point and a status per track, and which observations are
    still in use (an observation dropped as an outlier stays dropped)."""

    def __init__(self, scene, threshold: float, refine_steps: int, min_angle_deg: float, bundle_solver: str = "dense",
                 bundle_loss: str = "squared", bundle_loss_scale: float = 2.0, triangulation: str = "plain"):
        self.bundle_solver = bundle_solver
        self.triangulation = triangulation
        # a squared loss is the call without a loss: the scale has no effect on it
        self.loss = {} if bundle_loss == "squared" else dict(loss=bundle_loss, loss_scale=bundle_loss_scale)
        self.adjusted = np.zeros(0, dtype=np.int64)   # the observations of the last adjustment
        self.K = scene["K"]
        self.cam, self.pt, self.uv = scene["camera_indices"], scene["point_indices"], scene["pixels"]
        self.views = int(self.cam.max()) + 1
        self.P = int(self.pt.max()) + 1
        self.poses = np.zeros((self.views, 12))
        self.registered: list = []
        self.X = np.full((self.P, 3), np.nan)
        self.status = np.full(self.P, device.TRACKS_FEW_VIEWS, dtype=np.uint8)
        self.active = np.ones(len(self.cam), dtype=bool)
        self.threshold, self.refine_steps, self.min_angle_deg = threshold, refine_steps, min_angle_deg

    def in_registered(self) -> np.ndarray:
        return self.active & np.isin(self.cam, self.registered)

    def triangulate(self, points: np.ndarray):
        """(Re-)triangulate `points` from their active observations in registered views; observations above the threshold
        are dropped and the points they belonged to re-triangulated once.  With ``triangulation="robust"``: one robust call
        instead, and the observations it flags 0 on points that got an estimate become inactive."""
        if self.triangulation == "robust":
            use = self.in_registered() & np.isin(self.pt, points)
            if not use.any():
                return
            idx = np.nonzero(use)[0]
            r = triangulate_tracks_robust(self.K, self.poses, self.cam[idx], self.pt[idx], self.uv[idx], self.threshold,
                                          num_points=self.P, min_angle_deg=self.min_angle_deg, refine_steps=self.refine_steps)
            self.X[points], self.status[points] = r.points[points], r.status[points]
            self.active[idx[~np.isnan(r.observation_error) & ~r.inlier]] = False
            return
        for attempt in range(2):
            use = self.in_registered() & np.isin(self.pt, points)
            if not use.any():
                return
            idx = np.nonzero(use)[0]
            r = triangulate_tracks(self.K, self.poses, self.cam[idx], self.pt[idx], self.uv[idx], num_points=self.P,
                                   min_angle_deg=self.min_angle_deg, max_reprojection_error=self.threshold,
                                   refine_steps=self.refine_steps)
            self.X[points], self.status[points] = r.points[points], r.status[points]
            bad = idx[~np.isnan(r.observation_error) & ~(r.observation_error <= self.threshold)]
            if attempt == 1 or len(bad) == 0:
                return
            self.active[bad] = False
            points = np.unique(self.pt[bad])

    def start(self, obs: np.ndarray, max_steps: int):
        """The first points and the first adjustment: the tracks of the observations ``obs`` triangulated without the error
        check, the registered views adjusted on them, then every track triangulated with the checks.  Returns the
        adjustment's info."""
        r = triangulate_tracks(self.K, self.poses, self.cam[obs], self.pt[obs], self.uv[obs], num_points=self.P,
                               min_angle_deg=self.min_angle_deg, refine_steps=self.refine_steps)
        self.X, self.status = r.points, np.where(r.status == device.TRACKS_LARGE_ERROR, device.TRACKS_OK, r.status)
        info, _ = self.adjust(max_steps, drop=False)
        self.status[:] = device.TRACKS_FEW_VIEWS
        self.triangulate(self.pending())
        return info

    def pending(self) -> np.ndarray:
        """Tracks that are not OK and have at least two active observations in registered views."""
        use = self.in_registered()
        counts = np.bincount(self.pt[use], minlength=self.P)
        return np.nonzero((self.status != device.TRACKS_OK) & (counts >= 2))[0]

    def drop_outliers(self):
        """Drop the active observations of OK points in registered views whose error is above the threshold."""
        use = np.nonzero(self.in_registered() & (self.status[self.pt] == device.TRACKS_OK))[0]
        e = _errors(self.K, self.poses, self.X, self.cam[use], self.pt[use], self.uv[use])
        self.active[use[~(e <= self.threshold)]] = False

    def adjust(self, max_steps: int, drop: bool = True, refine=()):
        """Bundle adjustment of the registered cameras (camera 0 fixed) and the OK points on their active observations
        (first, with ``drop``, without the observations above the threshold).  ``refine``: the intrinsics to free; the
        refined camera matrix then replaces ``self.K``."""
        if drop:
            self.drop_outliers()
        ok = np.nonzero(self.status == device.TRACKS_OK)[0]
        use = np.nonzero(self.in_registered() & (self.status[self.pt] == device.TRACKS_OK))[0]
        cam_slot = np.full(self.views, -1)
        cam_slot[self.registered] = np.arange(len(self.registered))
        pt_slot = np.full(self.P, -1)
        pt_slot[ok] = np.arange(len(ok))
        auto = self.bundle_solver == "auto" and len(self.registered) > DENSE_MAX_VIEWS
        solver = "iterative" if auto else "dense"
        poses, X, info = bundle_adjust(self.K, self.poses[self.registered], self.X[ok], cam_slot[self.cam[use]],
                                       pt_slot[self.pt[use]], self.uv[use], fixed_cameras=(0,), max_steps=max_steps,
                                       linear_solver=solver, refine_intrinsics=refine, **self.loss)
        if refine and info.status == device.BUNDLE_OK:
            self.K = info.camera_matrix
        self.poses[self.registered] = poses
        self.X[ok] = X
        self.adjusted = use
        return info, len(use)


def _verified_matches(K, pix_a, pix_b, m, sed_threshold: float, iterations: int, e_solver: str):
    """The matches m ((n, 2) local indices) that the essential-matrix RANSAC winner keeps (its sample and its survivors,
    taken by index from the engine's inlier mask), or None when no model wins."""
    from structure_from_motion_amd.epipolar import _engine
    from structure_from_motion_amd.ransac._device_route import run_pass
    from structure_from_motion_amd.ransac.ransac import ErrorAggregationMethod, aggregation_code

    n = len(m)
    if n < 8:
        return None
    corr = device.normalize_correspondences(device.to_device(pix_a[m[:, 0]]), device.to_device(pix_b[m[:, 1]]), K)
    ws = device.RansacWorkspace(1, n, iterations)
    _, _, philox = _engine.draw_samples(ws.S, n, iterations)
    run_pass(e_solver, ws, corr.reshape(1, n, 4), sed_threshold, int(0.4 * n), aggregation_code(ErrorAggregationMethod.RMS),
             philox)
    outcome = ws.outcome(0)
    if outcome.best_h < 0:
        return None
    return m[device.checked_mask(outcome.mask) > 0]


def global_rotations(graph, views: int, max_residual_deg: float):
    """Huber from the spanning tree, then Cauchy from Huber's result (``average_graph_rotations``): (the Cauchy result, the
    indices of the graph's pairs whose residual is above ``max_residual_deg``)."""
    huber = average_graph_rotations(graph, views, loss="huber", loss_scale_deg=1.0, max_steps=100)
    cauchy = average_graph_rotations(graph, views, loss="cauchy", loss_scale_deg=1.0, initial_rotations=huber.R, max_steps=100)
    return cauchy, inconsistent_pairs(cauchy, max_residual_deg)


def global_positions(graph, rotations, views: int, max_residual_deg: float):
    """Huber with the warm-up from the spanning tree, then Cauchy from Huber's result (``average_graph_translations``): (the
    Cauchy result, the indices of the graph's pairs whose residual is above ``max_residual_deg``)."""
    huber = average_graph_translations(graph, rotations, views, loss="huber", loss_scale_deg=2.0, max_steps=POSITION_STEPS)
    cauchy = average_graph_translations(graph, rotations, views, loss="cauchy", loss_scale_deg=2.0, warmup_steps=0,
                                        initial_positions=huber.c, max_steps=POSITION_STEPS)
    return cauchy, inconsistent_pairs(cauchy, max_residual_deg)


def pair_pose_errors(pose, pairs, poses_true) -> dict:
    """Median and largest rotation and translation-direction error in degrees of the pairwise poses with status "ok" against
    the scene's true poses (R | t rows): the true relative pose of pair (i, j) is R_j R_i^T, t_j - R_j R_i^T t_i."""
    rot, direction = [], []
    for q, (i, j) in enumerate(np.asarray(pairs).tolist()):
        if pose.status[q] != "ok":
            continue
        Ri, Rj = poses_true[i, :9].reshape(3, 3), poses_true[j, :9].reshape(3, 3)
        R = Rj @ Ri.T
        t = poses_true[j, 9:] - R @ poses_true[i, 9:]
        rot.append(np.degrees(rotation_angle(pose.R[q], R)))
        c = float(pose.t[q] @ t / np.linalg.norm(t))
        direction.append(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))
    if not rot:
        return dict(pairs=0)
    return dict(pairs=len(rot), rotation_median_deg=float(np.median(rot)), rotation_max_deg=float(np.max(rot)),
                direction_median_deg=float(np.median(direction)), direction_max_deg=float(np.max(direction)))


def tracks_from_matches(scene, sed_threshold: float, iterations: int, e_solver: str, seed: int, verify: str = "loop",
                        relative_pose: bool = False, rotations: str = "incremental", drop_inconsistent_deg=None,
                        positions: str = "incremental", refine_pairs: int = 0):
    """The scene's tracks rebuilt from verified pairwise matches: (scene with the built camera_indices, point_indices and
    pixels, the build's info, the fraction of OK tracks whose features all belong to one true point, pairs kept, and with
    ``verify="batched"`` the number of pairs of each kind and the ``ViewGraph`` (with poses if ``relative_pose``), else None
    twice; with ``rotations="global"`` the result of ``global_rotations``, else None; with ``positions="global"`` the result
    of ``global_positions``, else None; with ``refine_pairs`` rounds of ``refine_relative_poses`` on the graph's poses, which
    every later stage then sees refined, ``pair_pose_errors`` before and after them, else None).  ``drop_inconsistent_deg``
    drops the inconsistent pairs before the build."""
    K = scene["K"]
    random.seed(seed)   # the pairs' RANSAC samples
    pm = synthetic.pairwise_matches(scene, seed=seed)
    pairs, kept, kinds, graph, averaged, positioned, pair_errors = [], [], None, None, None, None, None
    if verify == "batched":
        pose = dict(relative_pose=True) if relative_pose or rotations == "global" or refine_pairs > 0 else {}
        graph = verify_pairs(K, pm["features"], pm["pairs"], pm["matches"], sed_threshold, min_extra_fraction=0.4,
                             max_iterations=iterations, **pose)
        if refine_pairs > 0:
            refined = refine_relative_poses(K, pm["features"], graph, pm["matches"], sed_threshold, rounds=refine_pairs)
            pair_errors = dict(before=pair_pose_errors(graph.pose, graph.pairs, scene["poses_true"]),
                               after=pair_pose_errors(refined.graph.pose, graph.pairs, scene["poses_true"]),
                               rounds_kept=int(refined.accepted.sum()), lm_steps=int(refined.lm_steps.sum()))
            graph = refined.graph
        kinds = {kind: graph.kind.count(kind) for kind in ("essential", "homography", "none")}
        dropped = set()
        if rotations == "global":
            limit = INCONSISTENT_DEG if drop_inconsistent_deg is None else drop_inconsistent_deg
            averaged = global_rotations(graph, len(pm["features"]), limit)
            if positions == "global":
                positioned = global_positions(graph, averaged[0], len(pm["features"]), limit)
            if drop_inconsistent_deg is not None:
                dropped = set(averaged[1].tolist())
        for q, ((i, j), kind, inliers) in enumerate(zip(pm["pairs"], graph.kind, graph.inlier_matches)):
            if kind != "none" and q not in dropped:   # a pair without a model is dropped
                pairs.append((i, j))
                kept.append(inliers)
    else:
        for (i, j), m in zip(pm["pairs"], pm["matches"]):
            inliers = _verified_matches(K, pm["features"][i], pm["features"][j], m, sed_threshold, iterations, e_solver)
            if inliers is None:
                continue   # a pair without a model is dropped
            pairs.append((i, j))
            kept.append(inliers)
    r = build_tracks(pm["features"], np.array(pairs, dtype=np.int64).reshape(-1, 2), kept)
    truth = np.concatenate(pm["feature_points"])[r.feature_indices]
    lo = np.full(r.info.tracks, np.iinfo(np.int64).max)
    hi = np.full(r.info.tracks, -1)
    np.minimum.at(lo, r.point_indices, truth)
    np.maximum.at(hi, r.point_indices, truth)
    pure = float(np.mean(lo == hi)) if r.info.tracks else float("nan")
    built = dict(scene, camera_indices=r.camera_indices, point_indices=r.point_indices, pixels=r.pixels)
    return built, r.info, pure, len(pairs), kinds, graph, averaged, positioned, pair_errors


def run(views: int = 8, points: int = 2000, seed: int = 21, noise_px: float = 0.5, outlier_fraction: float = 0.2,
        sed_threshold: float = 6e-6, reprojection_threshold: float = 16.0, iterations: int = 2000, refine_steps: int = 10,
        ba_steps: int = 20, final_ba_steps: int = 50, step_deg: float = 5.0, bundle_solver: str = "dense",
        details: bool = False, pnp_solver: str | None = None, e_solver: str = "eight_point", tracks: str = "given",
        bundle_loss: str = "squared", bundle_loss_scale: float = 2.0, verify: str = "loop", seed_pair: str = "first",
        seed_min_angle_deg: float = 2.0, rotations: str = "incremental", drop_inconsistent_pairs_deg=None,
        positions: str = "incremental", register: str = "incremental", focal_error: float = 0.0,
        bundle_refine=(), refine_pairs: int = 0, triangulation: str = "plain") -> dict:
    if triangulation not in TRIANGULATIONS:
        raise ValueError(f"triangulation must be one of {TRIANGULATIONS}, got {triangulation!r}")
    if register not in REGISTER_ROUTES:
        raise ValueError(f"register must be one of {REGISTER_ROUTES}, got {register!r}")
    if pnp_solver is None:   # unset: the six-point DLT, as ever; the batched route is P3P
        pnp_solver = "p3p" if register == "batched" else "dlt"
    if pnp_solver not in ("dlt", "p3p"):
        raise ValueError(f"pnp_solver must be 'dlt' or 'p3p', got {pnp_solver!r}")
    if register == "batched" and pnp_solver != "p3p":
        raise ValueError("register='batched' registers every view with P3P (register_views): pnp_solver='dlt' is not supported there")
    if e_solver not in ("eight_point", "five_point"):
        raise ValueError(f"e_solver must be 'eight_point' or 'five_point', got {e_solver!r}")
    if tracks not in TRACK_SOURCES:
        raise ValueError(f"tracks must be one of {TRACK_SOURCES}, got {tracks!r}")
    if verify not in VERIFY_ROUTES:
        raise ValueError(f"verify must be one of {VERIFY_ROUTES}, got {verify!r}")
    if seed_pair not in SEED_PAIRS:
        raise ValueError(f"seed_pair must be one of {SEED_PAIRS}, got {seed_pair!r}")
    if rotations not in ROTATION_ROUTES:
        raise ValueError(f"rotations must be one of {ROTATION_ROUTES}, got {rotations!r}")
    if rotations == "global" and not (tracks == "matches" and verify == "batched"):
        raise ValueError("rotations='global' needs tracks='matches' and verify='batched'")
    if positions not in POSITION_ROUTES:
        raise ValueError(f"positions must be one of {POSITION_ROUTES}, got {positions!r}")
    if positions == "global" and rotations != "global":
        raise ValueError("positions='global' needs rotations='global'")
    if register == "global" and positions != "global":
        raise ValueError("register='global' needs positions='global'")
    if drop_inconsistent_pairs_deg is not None:
        if rotations != "global":
            raise ValueError("drop_inconsistent_pairs_deg needs rotations='global'")
        if not (np.isfinite(drop_inconsistent_pairs_deg) and drop_inconsistent_pairs_deg > 0.0):
            raise ValueError(f"drop_inconsistent_pairs_deg must be finite and positive, got {drop_inconsistent_pairs_deg!r}")
    if isinstance(refine_pairs, bool) or not isinstance(refine_pairs, int) or refine_pairs < 0:
        raise ValueError(f"refine_pairs must be a non-negative int, got {refine_pairs!r}")
    if refine_pairs > 0 and not (tracks == "matches" and verify == "batched"):
        raise ValueError("refine_pairs needs tracks='matches' and verify='batched'")
    auto_seed = seed_pair == "auto"
    if auto_seed and not (tracks == "matches" and verify == "batched"):
        raise ValueError("seed_pair='auto' needs tracks='matches' and verify='batched'")
    if bundle_solver not in BUNDLE_SOLVERS:
        raise ValueError(f"bundle_solver must be one of {BUNDLE_SOLVERS}, got {bundle_solver!r}")
    if bundle_loss not in BUNDLE_LOSSES:
        raise ValueError(f"bundle_loss must be one of {BUNDLE_LOSSES}, got {bundle_loss!r}")
    if not (np.isfinite(bundle_loss_scale) and _native.loss_scale_ok(bundle_loss_scale)):
        raise ValueError(f"bundle_loss_scale must be positive with a normal finite square, got {bundle_loss_scale!r}")
    limit = DENSE_MAX_VIEWS if bundle_solver == "dense" else MAX_VIEWS
    if not 2 <= views <= limit:
        raise ValueError(f"between 2 and {limit} views are supported with bundle_solver={bundle_solver!r}, got {views}")
    bundle_refine = tuple(bundle_refine) if not isinstance(bundle_refine, str) else bundle_refine
    if _native.bundle_refine_mask(bundle_refine) and views > DENSE_MAX_VIEWS:
        raise ValueError(f"bundle_refine needs the dense solver: at most {DENSE_MAX_VIEWS} views, got {views}")
    if not (np.isfinite(focal_error) and focal_error > -1.0):
        raise ValueError(f"focal_error must be a finite fraction above -1, got {focal_error!r}")
    scene = synthetic.multi_view_scene(views, points, seed, noise_px, outlier_fraction, step_deg=step_deg)
    K_true = scene["K"]
    if focal_error != 0.0:   # every stage sees the wrong camera matrix
        K_wrong = np.array(K_true, dtype=np.float64)
        K_wrong[:2, :2] *= 1.0 + focal_error
        scene = dict(scene, K=K_wrong)
    build, graph, averaged, positioned, pair_errors = None, None, None, None, None
    if tracks == "matches":
        scene, build_info, pure, kept_pairs, kinds, graph, averaged, positioned, pair_errors = tracks_from_matches(
            scene, sed_threshold, iterations, e_solver, seed, verify, relative_pose=auto_seed, rotations=rotations,
            drop_inconsistent_deg=drop_inconsistent_pairs_deg, positions=positions, refine_pairs=refine_pairs)
        build = dict(pairs_kept=kept_pairs, components=build_info.components, tracks=build_info.tracks,
                     observations=build_info.observations, conflicts=build_info.conflicts,
                     unmatched=build_info.unmatched, pure_track_fraction=pure)
        if kinds is not None:
            build.update(pairs_essential=kinds["essential"], pairs_homography=kinds["homography"], pairs_none=kinds["none"])
    K = scene["K"]
    rec = Reconstruction(scene, reprojection_threshold, refine_steps, min_angle_deg=1.0, bundle_solver=bundle_solver,
                         bundle_loss=bundle_loss, bundle_loss_scale=float(bundle_loss_scale), triangulation=triangulation)
    cam, pt, uv = rec.cam, rec.pt, rec.uv
    random.seed(seed)

    # 1. seed on views 0 and 1, or on the pair the view graph recommends
    va, vb, seed_q = 0, 1, None
    if auto_seed:
        seed_q = choose_seed_pair(graph, min_count=MIN_PNP_INLIERS, min_angle_deg=seed_min_angle_deg)
        va, vb = (int(v) for v in graph.pairs[seed_q])
    if register == "global":
        # every registered view starts at its global pose, in the gauge of view va and in units of the baseline va - vb
        P = global_poses(averaged[0], positioned[0])
        ok = np.nonzero(~np.isnan(P).any(axis=(1, 2)))[0]
        if not (np.isin([va, vb], ok).all()):
            raise ValueError(f"register='global' needs views {va} and {vb} registered in the global poses")
        Rg, cg = averaged[0].R, positioned[0].c
        base = float(np.linalg.norm(cg[vb] - cg[va]))
        for v in ok:
            Rv = Rg[v] @ Rg[va].T
            rec.poses[v] = _pose(Rv, -Rv @ (Rg[va] @ (cg[v] - cg[va]) / base))
        rec.registered = [va] + [int(v) for v in ok if v != va]
        first = rec.start(np.nonzero(rec.in_registered())[0], final_ba_steps)
        log = [dict(view=rec.registered[-1], points_ok=int(np.count_nonzero(rec.status == device.TRACKS_OK)))]
    else:
        in0 = np.full(rec.P, -1)
        in1 = np.full(rec.P, -1)
        in0[pt[cam == va]] = np.nonzero(cam == va)[0]
        in1[pt[cam == vb]] = np.nonzero(cam == vb)[0]
        both = np.nonzero((in0 >= 0) & (in1 >= 0))[0]
        if auto_seed:
            # the pair's pose is the one its inliers voted for in the verify_pairs call; the tracks through both views were
            # built from verified matches, so all of them start the reconstruction
            R1, t1, kept = graph.pose.R[seed_q], graph.pose.t[seed_q], both
        else:
            fa = [Feature(float(x), float(y)) for x, y in uv[in0[both]]]
            fb = [Feature(float(x), float(y)) for x, y in uv[in1[both]]]
            # RANSAC keeps the lowest-error model among those with enough extra inliers: asking for 40 % of the pairs keeps a
            # model fitted to a few outliers from winning (about 64 % of the pairs are clean at 20 % outliers per view)
            e, pairs = estimate_essential_mat_with_ransac(K, fa, fb, create_trivial_matches(len(both)),
                                                          sed_inlier_threshold=sed_threshold,
                                                          min_num_extra_inliers=int(0.4 * len(both)), max_iterations=iterations,
                                                          solver=e_solver)
            R1, t1, _ = recover_r_t_from_e(e, K, [p[0] for p in pairs], [p[1] for p in pairs])
            index_of = {(f.x, f.y): k for k, f in enumerate(fa)}
            kept = both[sorted(index_of[(p[0].x, p[0].y)] for p in pairs)]
        rec.poses[va] = _pose(np.eye(3), np.zeros(3))
        rec.poses[vb] = _pose(R1, t1)
        rec.registered = [va, vb]
        # The RANSAC winner is a minimal fit to one sample: with 5 degrees between the views its pose can be off by a few
        # hundredths of a radian, enough to push most two-view points over the threshold.  So the pairs E keeps are
        # triangulated without the error check first and the two views are adjusted on them; then every track is
        # triangulated with the checks.
        rec.start(np.nonzero(np.isin(pt, kept) & ((cam == va) | (cam == vb)))[0], final_ba_steps)
        log = [dict(view=vb, points_ok=int(np.count_nonzero(rec.status == device.TRACKS_OK)))]

    # 2.-4. register the view with the most observations of OK points, triangulate, adjust (with register="global" every
    # view is registered already)
    round_sizes = []
    while register == "batched" and len(rec.registered) < views:
        use = rec.active & (rec.status[pt] == device.TRACKS_OK)
        counts = np.bincount(cam[use], minlength=views)
        counts[rec.registered] = -1
        candidates = np.nonzero(counts >= MIN_PNP_INLIERS)[0]
        if len(candidates) == 0:
            break
        slot = np.full(views, -1)
        slot[candidates] = np.arange(len(candidates))
        obs = np.nonzero(use & (slot[cam] >= 0))[0]
        found = register_views(K, rec.X, slot[cam[obs]], pt[obs], uv[obs], reprojection_threshold, num_views=len(candidates),
                               min_num_extra_inliers=10, min_extra_fraction=BATCHED_MIN_EXTRA_FRACTION, max_iterations=iterations,
                               refine_rounds=2)
        accepted = [k for k in range(len(candidates)) if found.status[k] == "ok" and found.inlier_count[k] >= MIN_PNP_INLIERS]
        if not accepted:
            break
        for k in accepted:
            rec.poses[candidates[k]] = found.poses[k]
            rec.registered.append(int(candidates[k]))
        rec.triangulate(rec.pending())
        info, _ = rec.adjust(ba_steps)
        round_sizes.append(len(accepted))
        log.append(dict(round=len(round_sizes), views=[int(candidates[k]) for k in accepted],
                        pnp_inliers=[int(found.inlier_count[k]) for k in accepted],
                        points_ok=int(np.count_nonzero(rec.status == device.TRACKS_OK)), ba_status=info.status))
    while register == "incremental" and len(rec.registered) < views:
        use = rec.active & (rec.status[pt] == device.TRACKS_OK)
        counts = np.bincount(cam[use], minlength=views)
        counts[rec.registered] = -1
        v = int(np.argmax(counts))   # ties: the lower index
        obs = np.nonzero(use & (cam == v))[0]
        if len(obs) < MIN_PNP_INLIERS:
            break
        X = [rec.X[p] for p in pt[obs]]
        features = [Feature(float(x), float(y)) for x, y in uv[obs]]
        matches = [Match(a_index=i, b_index=i) for i in range(len(obs))]
        try:
            R, t, inliers = estimate_pose_pnp_with_ransac(K, X, features, matches, reprojection_threshold,
                                                          min_num_extra_inliers=10, max_iterations=iterations,
                                                          refine_rounds=2, solver=pnp_solver)
        except ValueError:
            break
        if len(inliers) < MIN_PNP_INLIERS:
            break
        rec.poses[v] = _pose(R, t)
        rec.registered.append(v)
        rec.triangulate(rec.pending())
        info, _ = rec.adjust(ba_steps)
        log.append(dict(view=v, pnp_inliers=len(inliers), points_ok=int(np.count_nonzero(rec.status == device.TRACKS_OK)),
                        ba_status=info.status))

    # 5. final bundle adjustment
    info, m = rec.adjust(final_ba_steps, refine=bundle_refine)
    if bundle_loss == "squared":
        sum_sq = info.final_cost
    else:   # final_cost is a sum of rho there: the squared errors of the adjusted observations
        a = rec.adjusted
        sum_sq = float(np.sum(_errors(rec.K, rec.poses, rec.X, cam[a], pt[a], uv[a])))
    truth = scene["poses_true"]
    if auto_seed:   # the gauge of the seed: the true poses relative to view va, in units of the pair's true baseline
        Ra, ta = truth[va, :9].reshape(3, 3), truth[va, 9:]
        Rv = np.einsum("vij,kj->vik", truth[:, :9].reshape(-1, 3, 3), Ra)   # R_v Ra^T
        truth = np.hstack([Rv.reshape(-1, 9), truth[:, 9:] - Rv @ ta])
    scale = float(np.linalg.norm(truth[vb, 9:]))
    rot_err = {int(v): rotation_angle(rec.poses[v, :9].reshape(3, 3), truth[v, :9].reshape(3, 3)) for v in rec.registered}
    t_err = {int(v): float(np.linalg.norm(rec.poses[v, 9:] - truth[v, 9:] / scale)) for v in rec.registered}
    out = {
        "views": views,
        "points": points,
        "views_registered": len(rec.registered),
        "registration_order": [int(v) for v in rec.registered],
        "rotation_error_rad": rot_err,
        "translation_error": t_err,
        "rms_px": float(np.sqrt(sum_sq / m)) if m else float("nan"),
        "ba_observations": m,
        "ba_status": info.status,
        "points_ok": int(np.count_nonzero(rec.status == device.TRACKS_OK)),
        "steps": log,
    }
    if focal_error != 0.0 or bundle_refine:
        out["focal"] = {"true": float(K_true[0, 0]), "error_before": float(abs(K[0, 0] / K_true[0, 0] - 1.0)),
                        "error_after": float(abs(rec.K[0, 0] / K_true[0, 0] - 1.0)),
                        "camera_matrix": [float(v) for v in np.asarray(rec.K).reshape(9)]}
    if triangulation != "plain":
        out["triangulation"] = triangulation
    if build is not None:
        out["track_build"] = build
    if auto_seed:
        out["seed_pair"] = [va, vb]
        out["median_angle_deg"] = float(graph.pose.median_angle_deg[seed_q])
    if pair_errors is not None:
        out["pair_refinement"] = pair_errors
    if averaged is not None:
        result, inconsistent = averaged
        # the gauge of the reconstruction: the true rotations above are relative to view va (its own when va is view 0)
        Rg = result.R @ result.R[va].T
        Rt = truth[:, :9].reshape(-1, 3, 3)
        Rt = Rt @ Rt[va].T
        out["global_rotations"] = {
            "rotation_error_rad": {int(v): rotation_angle(Rg[v], Rt[v]) for v in range(views) if result.registered[v]},
            "views_registered": int(np.count_nonzero(result.registered)),
            "status": result.status,
            "steps": result.steps,
            "cg_iterations": result.cg_iterations,
            "inconsistent_pairs": [[int(v) for v in graph.pairs[q]] for q in inconsistent],
            "pairs_dropped": len(inconsistent) if drop_inconsistent_pairs_deg is not None else 0,
        }
    if positioned is not None:
        result, off = positioned
        # the true centres in the gauge above, in units of the first pair's true baseline; the result turned into view va's
        # frame by its own global rotation, then scaled and shifted onto the truth
        Rt = truth[:, :9].reshape(-1, 3, 3)
        centres = -np.einsum("vji,vj->vi", Rt, truth[:, 9:] / scale)
        reg = np.nonzero(result.registered & averaged[0].registered)[0]
        mine = (result.c[reg] - result.c[reg].mean(axis=0)) @ averaged[0].R[va].T
        theirs = centres[reg] - centres[reg].mean(axis=0)
        s = float(np.sum(mine * theirs) / np.sum(mine * mine)) if len(reg) > 1 else 1.0
        out["global_positions"] = {
            "centre_error": {int(v): float(np.linalg.norm(s * mine[k] - theirs[k])) for k, v in enumerate(reg)},
            "views_registered": int(len(reg)),
            "status": result.status,
            "steps": result.steps,
            "cg_iterations": result.cg_iterations,
            "inconsistent_pairs": [[int(v) for v in graph.pairs[q]] for q in off],
        }
    if register == "batched":
        out["registration_rounds"] = {"solver": "p3p", "rounds": len(round_sizes), "views_per_round": round_sizes}
    if register == "global":
        out["bundle"] = {"initial_cost": float(first.initial_cost), "final_cost": float(first.final_cost)}
    if details:
        out["_scene"], out["_status"] = scene, rec.status.copy()
        if graph is not None:
            out["_graph"] = graph
        if positioned is not None:
            out["_rotations"], out["_positions"] = averaged[0], positioned[0]
    return out


def rotation_angle(Ra: np.ndarray, Rb: np.ndarray) -> float:
    """Angle in radians of Ra Rb^T."""
    c = (np.trace(Ra @ Rb.T) - 1.0) / 2.0
    return float(np.arccos(np.clip(c, -1.0, 1.0)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--views", type=int, default=8,
                    help=f"number of views (2 to {MAX_VIEWS}; to {DENSE_MAX_VIEWS} with --bundle-solver dense)")
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=21)
    ap.add_argument("--noise", type=float, default=0.5, help="pixel noise (standard deviation)")
    ap.add_argument("--outliers", type=float, default=0.2, help="fraction of observations replaced by random pixels")
    ap.add_argument("--sed-threshold", type=float, default=6e-6, help="two-view SED inlier threshold of the seed")
    ap.add_argument("--reprojection-threshold", type=float, default=16.0,
                    help="PnP and track inlier threshold in pixels squared")
    ap.add_argument("--refine-steps", type=int, default=10, help="LM steps per triangulated point (0: linear only)")
    ap.add_argument("--step-deg", type=float, default=5.0, help="angle between neighbouring views on the arc (degrees)")
    ap.add_argument("--bundle-solver", choices=BUNDLE_SOLVERS, default="auto",
                    help="dense: at most 64 views; auto: the iterative solver above 64 registered cameras")
    ap.add_argument("--pnp-solver", choices=("dlt", "p3p"), default=None,
                    help="minimal solver that registers each further view: six-point DLT (the default) or P3P on four-item "
                         "samples; --register batched is P3P and refuses dlt")
    ap.add_argument("--tracks", choices=TRACK_SOURCES, default="given",
                    help="given: the scene's tracks; matches: tracks built from RANSAC-verified pairwise matches")
    ap.add_argument("--triangulation", choices=TRIANGULATIONS, default="plain",
                    help="plain: the N-view DLT of all observations, those above the threshold dropped and the point triangulated "
                         "once more; robust: per-track RANSAC in one call (triangulate_tracks_robust)")
    ap.add_argument("--verify", choices=VERIFY_ROUTES, default="loop",
                    help="with --tracks matches: loop: one essential-matrix RANSAC per pair; batched: all pairs in one "
                         "verify_pairs call (homography and five-point essential per pair)")
    ap.add_argument("--seed-pair", choices=SEED_PAIRS, default="first",
                    help="first: seed on views 0 and 1; auto (with --tracks matches --verify batched): on the pair the view "
                         "graph recommends")
    ap.add_argument("--seed-min-angle", type=float, default=2.0,
                    help="with --seed-pair auto: least median triangulation angle of the seed pair's inliers, in degrees")
    ap.add_argument("--rotations", choices=ROTATION_ROUTES, default="incremental",
                    help="global (with --tracks matches --verify batched): also average the verified pairs' relative rotations "
                         "into one rotation per view and report each view's error and the inconsistent pairs")
    ap.add_argument("--drop-inconsistent-pairs", type=float, default=None, metavar="DEG",
                    help="with --rotations global: drop the pairs whose rotation residual is above DEG degrees before build_tracks")
    ap.add_argument("--positions", choices=POSITION_ROUTES, default="incremental",
                    help="global (with --rotations global): also average the pairs' translation directions into one position "
                         "per view and report each view's centre error and the inconsistent pairs")
    ap.add_argument("--register", choices=REGISTER_ROUTES, default="incremental",
                    help="global (with --positions global): start the reconstruction from the global poses instead of a seed "
                         "pair and a PnP chain; batched: register every view that sees enough points in one register_views "
                         "call per round (P3P)")
    ap.add_argument("--e-solver", choices=("eight_point", "five_point"), default="eight_point",
                    help="minimal solver of the two-view seed: eight-point, or five-point on six-item samples")
    ap.add_argument("--bundle-loss", choices=BUNDLE_LOSSES, default="squared",
                    help="loss of every bundle adjustment: squared, huber or cauchy")
    ap.add_argument("--bundle-loss-scale", type=float, default=2.0, help="scale of a huber or cauchy loss in pixels")
    ap.add_argument("--focal-error", type=float, default=0.0,
                    help="run the pipeline with a camera matrix whose focal lengths are this fraction off (0.05: 5 %% too long)")
    ap.add_argument("--bundle-refine", default="", metavar="focal[,principal_point]",
                    help="intrinsics the final bundle adjustment refines (at most 64 views)")
    ap.add_argument("--refine-pairs", type=int, default=0, metavar="K",
                    help="refine every pair's relative pose on its inliers with up to K rounds (0: off; needs --tracks matches "
                         "--verify batched); reports the pairwise pose errors against the truth before and after")
    args = ap.parse_args()
    if args.refine_pairs < 0 or (args.refine_pairs > 0 and not (args.tracks == "matches" and args.verify == "batched")):
        ap.error("--refine-pairs needs a non-negative K and, above 0, --tracks matches --verify batched")
    refine = tuple(name for name in args.bundle_refine.split(",") if name)
    try:
        _native.bundle_refine_mask(refine)
    except ValueError as e:
        ap.error(f"--bundle-refine: {e}")
    if refine and args.views > DENSE_MAX_VIEWS:
        ap.error(f"--bundle-refine needs at most {DENSE_MAX_VIEWS} views")
    if not (np.isfinite(args.focal_error) and args.focal_error > -1.0):
        ap.error("--focal-error must be a finite fraction above -1")
    limit = DENSE_MAX_VIEWS if args.bundle_solver == "dense" else MAX_VIEWS
    if not 2 <= args.views <= limit:
        ap.error(f"--views must be between 2 and {limit} with --bundle-solver {args.bundle_solver}")
    if args.seed_pair == "auto" and not (args.tracks == "matches" and args.verify == "batched"):
        ap.error("--seed-pair auto needs --tracks matches --verify batched")
    if args.rotations == "global" and not (args.tracks == "matches" and args.verify == "batched"):
        ap.error("--rotations global needs --tracks matches --verify batched")
    if args.positions == "global" and args.rotations != "global":
        ap.error("--positions global needs --rotations global")
    if args.register == "global" and args.positions != "global":
        ap.error("--register global needs --positions global")
    if args.register == "batched" and args.pnp_solver == "dlt":
        ap.error("--register batched registers every view with P3P: --pnp-solver dlt is not supported there")
    if args.drop_inconsistent_pairs is not None and not (args.rotations == "global" and args.drop_inconsistent_pairs > 0):
        ap.error("--drop-inconsistent-pairs needs --rotations global and a positive angle")
    print(json.dumps(run(args.views, args.points, args.seed, args.noise, args.outliers, sed_threshold=args.sed_threshold,
                         reprojection_threshold=args.reprojection_threshold, refine_steps=args.refine_steps,
                         step_deg=args.step_deg, bundle_solver=args.bundle_solver, pnp_solver=args.pnp_solver,
                         e_solver=args.e_solver, tracks=args.tracks, bundle_loss=args.bundle_loss,
                         bundle_loss_scale=args.bundle_loss_scale, verify=args.verify, seed_pair=args.seed_pair,
                         seed_min_angle_deg=args.seed_min_angle, rotations=args.rotations,
                         drop_inconsistent_pairs_deg=args.drop_inconsistent_pairs, positions=args.positions,
                         register=args.register, focal_error=args.focal_error, bundle_refine=refine,
                         refine_pairs=args.refine_pairs, triangulation=args.triangulation)))


if __name__ == "__main__":
    main()
