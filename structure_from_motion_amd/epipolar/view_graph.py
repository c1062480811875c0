"""Two-view verification of every image pair of a match graph in one device call: per pair the RANSAC
homography, the RANSAC five-point essential matrix on the same samples, both inlier lists and which of the two explains the
pair — what ``homography.select_two_view_model`` answers for one pair, for all pairs of ``build_tracks``'s input at once
(csrc/sfm_view_graph.hip, ``device.ViewGraphWorkspace``).  ``choose_seed_pair`` then picks the pair a reconstruction should
start from: a pure rotation or a plane fits an essential matrix to every match and would win on the essential count alone.
With ``relative_pose=True`` the same device calls also give how the two cameras of each pair stand to each other and the
median triangulation angle of its inliers (csrc/sfm_view_graph_pose.hip), which ``choose_seed_pair`` can gate
on: a pair with many inliers and a fraction of a degree of parallax is a poor place to start.  That pose is fitted to the five
items of a sample; ``refine_pose_rounds`` / ``refine_relative_poses`` refine it on the pair's inliers (DESIGN.md §6ac,
csrc/sfm_view_graph_refine.hip) before the averaging solvers and the seed pair see it."""
from __future__ import annotations

import os
import random
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import numpy.typing as npt

from .._native import POSE_STATUS as _POSE_STATUS   # PairPoses.status names by SFM_POSE_* code
from ..multiview.tracks import _feature_pixels, _pair_matches
from ..ransac.ransac import DEFAULT_MAX_ITERATIONS, ErrorAggregationMethod, aggregation_code
from .homography import MAX_HOMOGRAPHY_RATIO, check_camera_matrix

MAX_PAIRS_PER_CALL = 65535          # the grid's y extent: one sfm_verify_pairs call takes no more
BYTES_PER_PAIR_HYPOTHESIS = 224     # S 32, H and E 72 each, two sets of flags / cnt / s1 / s2 at 24


class PairPoses(NamedTuple):
    """The relative pose of each pair from its winning essential matrix (whatever the pair's kind) and the cheirality vote of
    that matrix's inliers: ``x_b ~ R x_a + t``."""
    R: npt.NDArray                     # (Q, 3, 3), NaN unless status is "ok"
    t: npt.NDArray                     # (Q, 3) unit length, NaN unless status is "ok"
    votes: npt.NDArray                 # (Q, 4) inliers in front of both cameras per candidate (R1,t), (R1,-t), (R2,t), (R2,-t)
    in_front: npt.NDArray              # (Q,) the votes of the chosen candidate, 0 when there is none
    median_angle_deg: npt.NDArray      # (Q,) lower median of the angle between the two viewing rays of those inliers, NaN unless "ok"
    status: List[str]                  # per pair "ok", "no_model", "not_essential" or "no_vote"


class ViewGraph(NamedTuple):
    pairs: npt.NDArray                 # (Q, 2) image indices, as given
    kind: List[str]                    # per pair "essential", "homography" or "none"
    E: npt.NDArray                     # (Q, 3, 3), NaN where no essential matrix has enough inliers
    H: npt.NDArray                     # (Q, 3, 3), NaN where no homography has enough inliers
    essential_count: npt.NDArray       # (Q,) the winner's sample size plus its extra inliers, 0 without a winner
    homography_count: npt.NDArray      # (Q,)
    ratio: npt.NDArray                 # (Q,) homography_count / essential_count, inf when essential_count is 0
    essential_inliers: List[npt.NDArray]    # per pair (k, 2) rows of matches[q]: the sample first, then the survivors by index
    homography_inliers: List[npt.NDArray]
    inlier_matches: List[npt.NDArray]  # per pair the inliers of the model its kind names ((0, 2) for "none"): build_tracks's input
    pose: Optional[PairPoses] = None   # with relative_pose=True


class PairRefinement(NamedTuple):
    """What ``refine_relative_poses`` returns: the graph with the refined poses and the record of each pair."""
    graph: ViewGraph                   # ``graph.pose.R`` / ``.t`` refined where a round was kept; every other field as given
    start_error: npt.NDArray           # (Q,) RMS symmetric epipolar distance of the start pose over its start set, NaN without a pose
    error: npt.NDArray                 # (Q,) the same of the kept pose over its inliers
    start_count: npt.NDArray           # (Q,) matches within the threshold under the start pose
    count: npt.NDArray                 # (Q,) matches within the threshold under the kept pose
    accepted: npt.NDArray              # (Q,) rounds whose result was kept (0: the pose is the start pose)
    lm_steps: npt.NDArray              # (Q,) Levenberg-Marquardt trial steps over all rounds
    status: List[str]                  # per pair "ok", "no_pose" or "too_few"
    inlier_matches: List[npt.NDArray]  # per pair (k, 2) rows of matches[q] within the threshold under the kept pose, by index



def pair_min_extra(counts, min_num_extra_inliers=None, min_extra_fraction: float = 0.0) -> npt.NDArray:
    """The gate of each pair: ``max(min_num_extra_inliers (an int or one per pair), floor(min_extra_fraction * n_q))``."""
    counts = np.asarray(counts, dtype=np.int64)
    fraction = float(min_extra_fraction)
    if not (np.isfinite(fraction) and fraction >= 0.0):
        raise ValueError(f"min_extra_fraction must be finite and >= 0, got {min_extra_fraction!r}")
    given = np.zeros(len(counts), dtype=np.int64) if min_num_extra_inliers is None else np.asarray(min_num_extra_inliers)
    if given.ndim == 0:
        given = np.full(len(counts), given)
    if given.shape != counts.shape or not np.issubdtype(given.dtype, np.integer):
        raise ValueError(f"min_num_extra_inliers must be an int or one int per pair ({len(counts)})")
    return np.maximum(given.astype(np.int64), np.floor(fraction * counts).astype(np.int64))


def chunk_bounds(pairs: int, iterations: int, max_hypotheses_per_call: int) -> List[tuple]:
    """``[(q0, q1), ...]``: the pairs of each device call, at most ``max_hypotheses_per_call // iterations`` (at least one, at
    most 65 535) pairs each — the buffers of a call take about 224 bytes per pair-hypothesis."""
    if max_hypotheses_per_call < 1:
        raise ValueError(f"max_hypotheses_per_call must be positive, got {max_hypotheses_per_call!r}")
    per_call = MAX_PAIRS_PER_CALL if iterations <= 0 else min(MAX_PAIRS_PER_CALL, max(1, max_hypotheses_per_call // iterations))
    return [(q0, min(q0 + per_call, pairs)) for q0 in range(0, pairs, per_call)]


def _checked_graph(features: Sequence, pairs, matches: Sequence):
    """The checks of ``build_tracks`` on the same three arguments -> (pixels per image, (Q, 2) pairs, (n_q, 2) matches per pair)."""
    feats = [_feature_pixels(f, i) for i, f in enumerate(features)]
    pair_arr = np.asarray(pairs)
    if pair_arr.size == 0:
        pair_arr = np.zeros((0, 2), dtype=np.int64)
    if pair_arr.ndim != 2 or pair_arr.shape[1] != 2:
        raise ValueError(f"pairs must have shape (Q, 2), got {pair_arr.shape}")
    if not np.issubdtype(pair_arr.dtype, np.integer):
        raise ValueError(f"pairs must hold integers, got {pair_arr.dtype}")
    Q = pair_arr.shape[0]
    if len(matches) != Q:
        raise ValueError(f"matches must hold one entry per pair ({Q}), got {len(matches)}")
    if Q and (pair_arr.min() < 0 or pair_arr.max() >= len(feats)):
        raise ValueError(f"pairs must index images 0 .. {len(feats) - 1}")
    if Q and np.any(pair_arr[:, 0] == pair_arr[:, 1]):
        raise ValueError("a pair must join two different images")
    per_pair = [_pair_matches(m, q) for q, m in enumerate(matches)]
    if sum(len(m) for m in per_pair) >= 2**31:
        raise ValueError("matches must number fewer than 2^31")
    for (i, j), m in zip(pair_arr.tolist(), per_pair):
        if len(m) and (m.min() < 0 or m[:, 0].max() >= len(feats[i]) or m[:, 1].max() >= len(feats[j])):
            raise ValueError("a match indexes a feature outside its image")
    return feats, pair_arr.astype(np.int64), per_pair


def _refine_arguments(rounds, max_steps):
    """(rounds, max_steps) as ints, both >= 0 (``ValueError``)."""
    for name, value in (("rounds", rounds), ("max_steps", max_steps)):
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 0 or value > 2**31 - 1:
            raise ValueError(f"pose refinement: {name} must be an int in [0, 2^31), got {value!r}")
    return int(rounds), int(max_steps)


def _upload_graph(K, feats, pair_arr, per_pair):
    """One upload and one normalisation for all pairs -> (device, corr f64 [N,4] on it, offset (Q + 1,) on the host and on
    the device): the pairs' K-normalised correspondences concatenated in pair order."""
    import torch

    from .. import device

    dev = device.require_gpu()
    offset = np.zeros(len(per_pair) + 1, dtype=np.int64)
    offset[1:] = np.cumsum([len(m) for m in per_pair])
    pix = np.empty((2, int(offset[-1]), 2))
    for q, ((i, j), m) in enumerate(zip(pair_arr.tolist(), per_pair)):
        pix[0, offset[q]:offset[q + 1]] = feats[i][m[:, 0]]
        pix[1, offset[q]:offset[q + 1]] = feats[j][m[:, 1]]
    pix = device.to_device(pix)   # one upload: [2, N, 2]
    corr = device.normalize_correspondences(pix[0], pix[1], K)
    return dev, corr, offset, device.to_device(offset, torch.int64)


def verify_pairs(camera_matrix, features: Sequence, pairs, matches: Sequence, inlier_threshold: float,
                 min_num_extra_inliers=None, min_extra_fraction: float = 0.0, max_iterations: int | None = None,
                 max_homography_ratio: float = MAX_HOMOGRAPHY_RATIO, seed: int | None = None,
                 max_hypotheses_per_call: int = 2**21, relative_pose: bool = False,
                 distance_threshold: float = 50.0, refine_pose_rounds: int = 0, refine_pose_max_steps: int = 20) -> ViewGraph:
    """Verify all Q pairs of a match graph: ``features``, ``pairs`` and ``matches`` exactly as ``build_tracks`` takes them.

    Per pair, ``max_iterations`` Philox samples serve a homography pass (their first four items) and a five-point essential
    pass (their first six), both with ``inlier_threshold`` in K-normalised units, the RMS aggregation and the gate
    ``max(min_num_extra_inliers, floor(min_extra_fraction * n_q))`` (``min_num_extra_inliers``: an int or one per pair);
    degenerate samples never compete and never raise.  The kind of a pair is ``"none"`` when neither model has a winner,
    ``"homography"`` when E has none or ``homography_count / essential_count > max_homography_ratio``, else
    ``"essential"``.  A pair with fewer than four matches has no model, one with four or five a homography at most.

    Pair q draws its samples with ``seed + q`` (``seed``, else ``SFM_SEED``, else 64 bits of ``random``), so the result
    does not depend on how the pairs are split into device calls (``max_hypotheses_per_call`` pair-hypotheses each).  One
    upload and one normalisation serve all pairs.  Every argument is checked before any device work (``ValueError``).

    ``relative_pose=True`` adds ``pose`` (``PairPoses``): per pair with an essential winner the pose its inliers vote for among
    the four of that matrix (an inlier votes when it triangulates in front of both cameras within ``distance_threshold``), and
    the median angle between the viewing rays of the voters.  It needs ``max_iterations >= 1`` and changes no other field.

    ``refine_pose_rounds > 0`` (it needs ``relative_pose=True``) refines each of those poses on the pair's matches within
    ``inlier_threshold`` under it: up to that many rounds of at most ``refine_pose_max_steps`` Levenberg-Marquardt steps on the
    summed symmetric epipolar distance, a round kept when it has more inliers, or as many and a lower RMS error
    (``sfm_refine_pair_poses``).  ``pose.R`` and ``pose.t`` are then the refined ones; the votes, ``in_front`` and the median
    angle stay those of the start pose, and no other field changes.  ``refine_relative_poses`` also returns each pair's record."""
    K = check_camera_matrix(camera_matrix)
    refine_rounds, refine_steps = _refine_arguments(refine_pose_rounds, refine_pose_max_steps)
    if refine_rounds > 0 and not relative_pose:
        raise ValueError("refine_pose_rounds needs relative_pose=True")
    distance = float(distance_threshold)
    if not (np.isfinite(distance) and distance > 0.0):
        raise ValueError(f"distance_threshold must be finite and positive, got {distance_threshold!r}")
    feats, pair_arr, per_pair = _checked_graph(features, pairs, matches)
    Q = len(per_pair)
    counts = np.array([len(m) for m in per_pair], dtype=np.int64)
    gate = pair_min_extra(counts, min_num_extra_inliers, min_extra_fraction)
    iterations = DEFAULT_MAX_ITERATIONS if max_iterations is None else int(max_iterations)
    if relative_pose and iterations < 1:
        raise ValueError(f"relative_pose needs max_iterations >= 1, got {max_iterations!r}")
    chunks = chunk_bounds(Q, iterations, max_hypotheses_per_call)
    if seed is None:
        seed = int(os.environ["SFM_SEED"]) if "SFM_SEED" in os.environ else random.getrandbits(64)
    empty = np.zeros((0, 2), dtype=np.int64)
    if Q == 0:
        none = np.zeros((0, 3, 3))
        no_pose = PairPoses(none.copy(), np.zeros((0, 3)), np.zeros((0, 4), np.int64), np.zeros(0, np.int64), np.zeros(0), [])
        return ViewGraph(pair_arr, [], none, none.copy(), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0), [], [], [],
                         no_pose if relative_pose else None)
    from .. import device

    dev, corr, offset, offset_dev = _upload_graph(K, feats, pair_arr, per_pair)
    gate_dev = device.to_device(gate.astype(np.float64))
    aggregation = aggregation_code(ErrorAggregationMethod.RMS)
    outcomes = []
    for q0, q1 in chunks:
        lo, hi = int(offset[q0]), int(offset[q1])
        ws = device.ViewGraphWorkspace(q1 - q0, hi - lo, max(iterations, 0), dev)
        ws.run(corr[lo:hi], offset_dev[q0:q1 + 1] - lo, gate_dev[q0:q1], inlier_threshold, aggregation, max_homography_ratio,
               seed + q0, seed_stride=1)
        if relative_pose:
            ws.poses(distance)
        if refine_rounds > 0:
            ws.refine_poses(inlier_threshold, aggregation, refine_rounds, refine_steps)
        outcomes.append(ws.outcome())
    cat = lambda name: np.concatenate([getattr(o, name) for o in outcomes])   # noqa: E731
    code, h_mask, e_mask = cat("kind"), cat("homography_mask"), cat("essential_mask")
    if np.any(code == device.PAIR_BAD_OFFSETS):
        raise RuntimeError("verify_pairs: the device refused the offset table (SFM_PAIR_BAD_OFFSETS)")
    h_sample, e_sample = cat("homography_sample"), cat("essential_sample")

    def inliers(q, sample, mask):
        if sample[q, 0] < 0:
            return empty
        survivors = np.nonzero(mask[offset[q]:offset[q + 1]] == 1)[0]
        return per_pair[q][np.concatenate([sample[q], survivors])]

    h_in = [inliers(q, h_sample, h_mask) for q in range(Q)]
    e_in = [inliers(q, e_sample, e_mask) for q in range(Q)]
    kind = [device.PAIR_KINDS[c] for c in code]
    chosen = [e_in[q] if kind[q] == "essential" else (h_in[q] if kind[q] == "homography" else empty) for q in range(Q)]
    pose = None
    if relative_pose:
        votes, best = cat("pose_votes").astype(np.int64), cat("pose_best")
        in_front = np.where(best >= 0, votes[np.arange(Q), np.maximum(best, 0)], 0)
        pose = PairPoses(cat("pose_R"), cat("pose_t"), votes, in_front, np.degrees(cat("pose_median_angle")),
                         [device.POSE_STATUS[c] for c in cat("pose_status")])
    return ViewGraph(pair_arr, kind, cat("E"), cat("H"), cat("essential_count").astype(np.int64),
                     cat("homography_count").astype(np.int64), cat("ratio"), e_in, h_in, chosen, pose)


def refine_relative_poses(camera_matrix, features: Sequence, graph: ViewGraph, matches: Sequence, inlier_threshold: float,
                          rounds: int = 2, max_steps: int = 20) -> PairRefinement:
    """Refine the relative poses of ``graph`` (``verify_pairs(..., relative_pose=True)``) on the matches they were verified
    on: what ``refine_pose_rounds`` does inside ``verify_pairs``, on a graph that is already there, with each pair's record
    (``PairRefinement``).  ``features`` and ``matches`` as ``verify_pairs`` took them; the pairs are ``graph.pairs``.  Every
    argument is checked before any device work (``ValueError``)."""
    K = check_camera_matrix(camera_matrix)
    rounds, max_steps = _refine_arguments(rounds, max_steps)
    thr = float(inlier_threshold)
    if np.isnan(thr):
        raise ValueError("inlier_threshold must be a number")
    if graph.pose is None:
        raise ValueError("refine_relative_poses needs graph.pose: call verify_pairs with relative_pose=True")
    feats, pair_arr, per_pair = _checked_graph(features, graph.pairs, matches)
    Q = len(per_pair)
    pose = graph.pose
    if not (len(pose.status) == Q and np.shape(pose.R) == (Q, 3, 3) and np.shape(pose.t) == (Q, 3)):
        raise ValueError(f"graph.pose must hold one pose per pair ({Q})")
    unknown = sorted(set(pose.status) - set(_POSE_STATUS))
    if unknown:
        raise ValueError(f"graph.pose.status holds unknown names {unknown}")
    if Q == 0:
        none = np.zeros(0, np.int64)
        return PairRefinement(graph, np.zeros(0), np.zeros(0), none, none.copy(), none.copy(), none.copy(), [], [])
    import torch

    from .. import device

    table = np.zeros(Q, dtype=device.POSE_DTYPE)
    table["R"], table["t"], table["votes"] = pose.R, pose.t, pose.votes
    table["median_angle"] = np.radians(pose.median_angle_deg)
    table["status"] = [_POSE_STATUS.index(name) for name in pose.status]
    table["best"] = np.where(table["status"] == device.POSE_OK, np.argmax(table["votes"], axis=1), -1)
    dev, corr, offset, offset_dev = _upload_graph(K, feats, pair_arr, per_pair)
    aggregation = aggregation_code(ErrorAggregationMethod.RMS)
    tables, masks, infos = [], [], []
    for q0 in range(0, Q, MAX_PAIRS_PER_CALL):
        q1 = min(q0 + MAX_PAIRS_PER_CALL, Q)
        lo, hi = int(offset[q0]), int(offset[q1])
        pose_in = torch.from_numpy(table[q0:q1].view(np.uint8).reshape(q1 - q0, device.POSE_BYTES).copy()).to(dev)
        out, mask, info = device.refine_pair_poses(corr[lo:hi], offset_dev[q0:q1 + 1] - lo, pose_in, thr, aggregation, rounds,
                                                   max_steps)
        tables.append(out.cpu().numpy().reshape(-1).view(device.POSE_DTYPE))
        masks.append(mask.cpu().numpy())
        infos.append(device.read_pair_refine_info(info))
    refined, mask, info = np.concatenate(tables), np.concatenate(masks), np.concatenate(infos)
    inliers = [per_pair[q][np.nonzero(mask[offset[q]:offset[q + 1]])[0]] for q in range(Q)]
    new_pose = pose._replace(R=refined["R"].copy(), t=refined["t"].copy())
    return PairRefinement(graph._replace(pose=new_pose), info["start_error"].copy(), info["error"].copy(),
                          info["start_count"].astype(np.int64), info["count"].astype(np.int64), info["accepted"].astype(np.int64),
                          info["lm_steps"].astype(np.int64), [device.PAIR_REFINE_STATUS[c] for c in info["status"]], inliers)


def choose_seed_pair(graph: ViewGraph, min_count: int = 0, min_angle_deg: float = 0.0) -> int:
    """The pair a reconstruction should start from: among the pairs of kind ``"essential"`` with ``essential_count >=
    min_count`` the one with the largest ``essential_count``; ties go to the lower ratio, then to the lower index.
    With ``min_angle_deg > 0`` a candidate must also have pose status ``"ok"`` and ``median_angle_deg >= min_angle_deg``
    (``graph.pose`` must be there: ``verify_pairs(..., relative_pose=True)``).  ``ValueError`` when there is none."""
    gated = min_angle_deg > 0
    if gated and graph.pose is None:
        raise ValueError("min_angle_deg needs graph.pose: call verify_pairs with relative_pose=True")
    best = None
    for q, kind in enumerate(graph.kind):
        if kind != "essential" or graph.essential_count[q] < min_count:
            continue
        if gated and not (graph.pose.status[q] == "ok" and graph.pose.median_angle_deg[q] >= min_angle_deg):
            continue
        key = (-int(graph.essential_count[q]), float(graph.ratio[q]), q)
        if best is None or key < best:
            best = key
    if best is None:
        raise ValueError("no pair of kind 'essential' with enough inliers")
    return best[2]
