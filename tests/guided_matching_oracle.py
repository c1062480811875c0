"""NumPy definition of guided matching: match_pairs_guided_kernel of csrc/sfm_match_pairs.hip is
compared with it byte for byte.

The inputs of the graph matcher (tests/graph_matching_oracle.py), plus per feature its K-normalised coordinates ``xy float64
[n, 2]`` and per pair a ``model float64 (3, 3)``, a ``kind`` (0 none, 1 essential, 2 homography: the view graph's codes) and a
``threshold float64``.  For pair q = (i, j) a row a is a feature of image i and a column b one of image j.

  err(a, b)     kind 1: ``oracle.sfm_oracle.sed_values(model, (xa, ya, xb, yb))``, the symmetric epipolar distance; kind 2:
                ``homography_oracle.transfer_error(model, (xa, ya, xb, yb))``, the symmetric transfer error under the model and
                its adjugate.  Both in the operation order those functions document, and always with image i's feature as a —
                also while the column summary is built, so the two summaries agree on every (a, b) bit for bit.
  adm(a, b)     both features valid and err(a, b) <= threshold: one IEEE compare, false for NaN, so a NaN model, coordinate or
                threshold admits nothing.  Kind 0 admits nothing.  Any other kind is refused (``ValueError`` here, pair_status 1
                on the device).
  row summary   over the admissible columns of a: best_r[a] the smallest d(a, b), arg_r[a] the smallest such b, second_r[a] the
                smallest d over admissible b != arg_r[a], NONE when there is none.  The column summary swaps the roles, over
                the admissible rows of b.
  keep, output  exactly graph_matching_oracle's, on these summaries.

The transposition property of the graph matcher is not claimed: err(E, a, b) and err(E^T, b, a) round differently.
"""
import numpy as np

import graph_matching_oracle as gmo
import homography_oracle as ho
from oracle import sfm_oracle as orc

NONE = gmo.NONE
KIND_NONE, KIND_ESSENTIAL, KIND_HOMOGRAPHY = 0, 1, 2
KIND_CODES = {"none": KIND_NONE, "essential": KIND_ESSENTIAL, "homography": KIND_HOMOGRAPHY}


def errors(model, kind, xy_a, xy_b) -> np.ndarray:
    """[n_a, n_b] float64: err(a, b) of every pair of features under one model of kind 1 or 2."""
    xy_a, xy_b = np.asarray(xy_a, dtype=np.float64).reshape(-1, 2), np.asarray(xy_b, dtype=np.float64).reshape(-1, 2)
    n_a, n_b = len(xy_a), len(xy_b)
    corr = np.empty((n_a * n_b, 4))
    corr[:, :2] = np.repeat(xy_a, n_b, axis=0)
    corr[:, 2:] = np.tile(xy_b, (n_a, 1))
    model = np.asarray(model, dtype=np.float64).reshape(3, 3)
    with np.errstate(all="ignore"):
        e = orc.sed_values(model, corr) if kind == KIND_ESSENTIAL else ho.transfer_error(model.reshape(9), corr)
    return np.asarray(e).reshape(n_a, n_b)


def admissible(model, kind, threshold, xy_a, valid_a, xy_b, valid_b) -> np.ndarray:
    """[n_a, n_b] bool: adm(a, b)."""
    valid_a, valid_b = np.asarray(valid_a, dtype=bool), np.asarray(valid_b, dtype=bool)
    kind = int(kind)
    if kind not in (KIND_NONE, KIND_ESSENTIAL, KIND_HOMOGRAPHY):
        raise ValueError(f"unknown model kind {kind}")
    if kind == KIND_NONE:
        return np.zeros((len(valid_a), len(valid_b)), dtype=bool)
    with np.errstate(invalid="ignore"):
        within = errors(model, kind, xy_a, xy_b) <= np.float64(threshold)
    return within & valid_a[:, None] & valid_b[None, :]


def gated_summary(d, adm):
    """(best, arg, second) per row of the distance matrix ``d`` over the admissible columns: int64 [n_a]."""
    n_a = d.shape[0]
    best, arg, second = np.full(n_a, NONE, np.int64), np.full(n_a, -1, np.int64), np.full(n_a, NONE, np.int64)
    if n_a == 0 or d.shape[1] == 0:
        return best, arg, second
    masked = np.where(adm, d, NONE)
    first = np.argmin(masked, axis=1)
    rows = np.arange(n_a)
    lowest = masked[rows, first]
    masked[rows, first] = NONE
    runner_up = masked.min(axis=1)
    some = lowest != NONE
    best[some], arg[some], second[some] = lowest[some], first[some], runner_up[some]
    return best, arg, second


class Summaries:
    """Both summaries of one guided pair; ``graph_matching_oracle.decide`` takes it."""

    def __init__(self, d, adm):
        self.rows = gated_summary(d, adm)
        self.columns = gated_summary(d.T, adm.T)


def pair_summaries(image_a, image_b, model, kind, threshold, d=None) -> Summaries:
    """``image`` = (bits, valid, xy).  ``d`` may carry the distance matrix when the caller has it."""
    d = gmo.distances(image_a[0], image_b[0]) if d is None else d
    return Summaries(d, admissible(model, kind, threshold, image_a[2], image_a[1], image_b[2], image_b[1]))


def match_pair(image_a, image_b, model, kind, threshold, max_distance=64, ratio=0.8, cross_check=True):
    """(partner int32 [n_a], distance int32 [n_a]) of the rows of one pair."""
    return gmo.decide(pair_summaries(image_a, image_b, model, kind, threshold), max_distance, ratio, cross_check)


class GraphSummaries:
    """The summaries of every pair of a guided graph, computed once and shared by every choice of options.  ``images`` is a
    sequence of (bits, valid, xy); ``models`` (Q, 3, 3), ``kinds`` (Q,) codes, ``thresholds`` (Q,)."""

    def __init__(self, images, pairs, models, kinds, thresholds):
        self.pairs = [(int(i), int(j)) for i, j in np.asarray(pairs).reshape(-1, 2)]
        self.sizes = [len(im[1]) for im in images]
        matrices = {}
        self.per_pair = []
        for q, (i, j) in enumerate(self.pairs):
            lo, hi = min(i, j), max(i, j)
            if (lo, hi) not in matrices:
                matrices[lo, hi] = gmo.distances(images[lo][0], images[hi][0])
            d = matrices[lo, hi] if i < j else matrices[lo, hi].T
            self.per_pair.append(pair_summaries(images[i], images[j], models[q], kinds[q], thresholds[q], d))

    def rows(self, max_distance=64, ratio=0.8, cross_check=True):
        """(partner, distance) int32 over all pairs' rows, pair after pair, and the row offsets int64 [Q + 1]."""
        out = [gmo.decide(s, max_distance, ratio, cross_check) for s in self.per_pair]
        offset = np.zeros(len(self.pairs) + 1, dtype=np.int64)
        offset[1:] = np.cumsum([self.sizes[i] for i, _ in self.pairs])
        if not out:
            return np.zeros(0, np.int32), np.zeros(0, np.int32), offset
        return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out]), offset

    def matches(self, max_distance=64, ratio=0.8, cross_check=True):
        """(matches per pair, distances per pair)."""
        lists = [gmo.compact(*gmo.decide(s, max_distance, ratio, cross_check)) for s in self.per_pair]
        return [m for m, _ in lists], [d for _, d in lists]


def match_graph(images, pairs, models, kinds, thresholds, max_distance=64, ratio=0.8, cross_check=True):
    """(matches per pair, distances per pair) of a whole guided graph."""
    return GraphSummaries(images, pairs, models, kinds, thresholds).matches(max_distance, ratio, cross_check)
