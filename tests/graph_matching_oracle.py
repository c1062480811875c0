"""NumPy definition of the graph matcher: the HIP kernels of csrc/sfm_match_pairs.hip are compared
with it bit for bit.

Inputs: per image, descriptors ``bits uint8 [n, 32]`` and ``valid [n]``; ``pairs (Q, 2)``; the options ``max_distance`` (int,
0..256), ``ratio`` (float64 > 0, or None) and ``cross_check`` (bool).  For pair q = (i, j) the rows are the features of image i
and the columns the features of image j.

  d(a, b)       popcount of the XOR of the two 32-byte descriptors; defined only when both are valid.  An invalid feature never
                matches, and it is never anybody's best or runner-up.
  row summary   of a valid row a, when image j has a valid feature: best_r[a] = the smallest d(a, .); arg_r[a] = the smallest
                b that attains it; second_r[a] = the smallest d(a, b) over valid b != arg_r[a], NONE when there is no such b.
                A tie for the best gives second == best.
  column summary  best_c[b], arg_c[b] (the smallest a), second_c[b]: the same with the roles swapped.
  distinctive   d against a runner-up s: true when ratio is None or s is NONE, else float64(d) <= ratio * float64(s) — one IEEE
                multiply and one compare.
  keep          row a keeps b = arg_r[a] iff a is valid and image j has a valid feature, best_r[a] <= max_distance, best_r[a]
                is distinctive against second_r[a] and, with cross_check, arg_c[b] == a and best_r[a] is distinctive against
                second_c[b].
  output        per row partner int32 and distance int32, both -1 when nothing is kept; the matches of pair q are its kept
                rows in ascending a: an (n_q, 2) int64 array plus their distances.
"""
import numpy as np

NONE = 2**31 - 1   # no distance (no valid partner, or no runner-up)


def distances(bits_a, bits_b) -> np.ndarray:
    """[n_a, n_b] int64: the Hamming distance of every descriptor pair, whatever the validity flags say."""
    a = np.ascontiguousarray(bits_a, dtype=np.uint8).reshape(-1, 32).view(np.uint64)
    b = np.ascontiguousarray(bits_b, dtype=np.uint8).reshape(-1, 32).view(np.uint64)
    out = np.zeros((len(a), len(b)), dtype=np.int64)
    for w in range(4):
        out += np.bitwise_count(a[:, None, w] ^ b[None, :, w])
    return out


def row_summary(d, valid_a, valid_b):
    """(best, arg, second) per row of the distance matrix ``d``: int64 [n_a]; an invalid row, or one without a valid column,
    has best NONE and arg -1."""
    valid_a, valid_b = np.asarray(valid_a, dtype=bool), np.asarray(valid_b, dtype=bool)
    n_a, n_b = d.shape
    best, arg, second = np.full(n_a, NONE, np.int64), np.full(n_a, -1, np.int64), np.full(n_a, NONE, np.int64)
    if n_a == 0 or not valid_b.any():
        return best, arg, second
    masked = np.where(valid_b[None, :], d, NONE)
    first = np.argmin(masked, axis=1)                 # the smallest column that attains the minimum
    rows = np.arange(n_a)
    lowest = masked[rows, first]
    masked[rows, first] = NONE
    runner_up = masked.min(axis=1)
    best[valid_a], arg[valid_a], second[valid_a] = lowest[valid_a], first[valid_a], runner_up[valid_a]
    return best, arg, second


def distinctive(d, s, ratio):
    """Element-wise: d against the runner-up s."""
    d, s = np.asarray(d, dtype=np.int64), np.asarray(s, dtype=np.int64)
    if ratio is None:
        return np.ones(d.shape, dtype=bool)
    return (s == NONE) | (d.astype(np.float64) <= np.float64(ratio) * s.astype(np.float64))


class Summaries:
    """Both summaries of one ordered image pair: everything the options do not touch."""

    def __init__(self, bits_a, valid_a, bits_b, valid_b, d=None):
        d = distances(bits_a, bits_b) if d is None else d
        self.rows = row_summary(d, valid_a, valid_b)
        self.columns = row_summary(d.T, valid_b, valid_a)


def decide(summaries: Summaries, max_distance=64, ratio=0.8, cross_check=True):
    """(partner int32 [n_a], distance int32 [n_a]) from the two summaries."""
    best, arg, second = summaries.rows
    _, arg_c, second_c = summaries.columns
    keep = (best != NONE) & (best <= int(max_distance)) & distinctive(best, second, ratio)
    if cross_check and len(arg_c):
        b = np.maximum(arg, 0)
        keep &= (arg_c[b] == np.arange(len(best))) & distinctive(best, second_c[b], ratio)
    partner = np.where(keep, arg, -1).astype(np.int32)
    distance = np.where(keep, best, -1).astype(np.int32)
    return partner, distance


def match_pair(bits_a, valid_a, bits_b, valid_b, max_distance=64, ratio=0.8, cross_check=True):
    """(partner, distance) of the rows of one pair."""
    return decide(Summaries(bits_a, valid_a, bits_b, valid_b), max_distance, ratio, cross_check)


def compact(partner, distance):
    """The match list of one pair: ((n, 2) int64 of (a, b) in ascending a, (n,) int32 distances)."""
    a = np.nonzero(partner >= 0)[0]
    return np.column_stack([a, partner[a].astype(np.int64)]).astype(np.int64).reshape(-1, 2), distance[a]


class GraphSummaries:
    """The summaries of every pair of a graph, computed once and shared by every choice of options.  ``descriptors`` is a
    sequence of (bits, valid); the distance matrix of an unordered pair serves both of its orders."""

    def __init__(self, descriptors, pairs):
        self.pairs = [(int(i), int(j)) for i, j in np.asarray(pairs).reshape(-1, 2)]
        self.sizes = [len(d[1]) for d in descriptors]
        matrices, self.per_pair = {}, {}
        for i, j in self.pairs:
            if (i, j) in self.per_pair:
                continue
            lo, hi = min(i, j), max(i, j)
            if (lo, hi) not in matrices:
                matrices[lo, hi] = distances(descriptors[lo][0], descriptors[hi][0])
            d = matrices[lo, hi] if i < j else matrices[lo, hi].T
            self.per_pair[i, j] = Summaries(None, descriptors[i][1], None, descriptors[j][1], d)

    def rows(self, max_distance=64, ratio=0.8, cross_check=True):
        """(partner, distance) int32 over all pairs' rows, pair after pair, and the row offsets int64 [Q + 1]."""
        out = [decide(self.per_pair[p], max_distance, ratio, cross_check) for p in self.pairs]
        offset = np.zeros(len(self.pairs) + 1, dtype=np.int64)
        offset[1:] = np.cumsum([self.sizes[i] for i, _ in self.pairs])
        if not out:
            return np.zeros(0, np.int32), np.zeros(0, np.int32), offset
        return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out]), offset

    def matches(self, max_distance=64, ratio=0.8, cross_check=True):
        """(matches per pair, distances per pair)."""
        lists = [compact(*decide(self.per_pair[p], max_distance, ratio, cross_check)) for p in self.pairs]
        return [m for m, _ in lists], [d for _, d in lists]


def match_graph(descriptors, pairs, max_distance=64, ratio=0.8, cross_check=True):
    """(matches per pair, distances per pair) of a whole graph."""
    return GraphSummaries(descriptors, pairs).matches(max_distance, ratio, cross_check)
