"""Fixtures and the stream case of guided matching (sfm_match_pairs_guided).

``collection(family)`` is the collection of the parity tests: the eight image sizes and the three descriptor families of
tests/test_gpu_graph_matching.py, coordinates from a seeded two-view scene mixed with uniform ones, and per pair a model, a
kind and a threshold that cycle through every combination.  ``repeated_chain`` is the NumPy chain of the accuracy conditions.

Importing this module registers the stream case of the new entry point in ``stream_cases.CASES``; the two test files of the
feature import it at their top and sort before test_gpu_streams.py and test_stream_cases_host.py, so both of those see the
complete table in a run of the whole suite."""
import functools

import numpy as np

import graph_matching_oracle as gmo
import guided_matching_oracle as go
import homography_oracle as ho
import stream_cases
from structure_from_motion_amd import synthetic

# no features, one, two, a row block less one / exactly / plus one (256), an LDS tile plus one (512), two tiles and five row blocks
SIZES = (0, 1, 2, 255, 256, 257, 513, 1030)
ALL_INVALID, ONE_VALID = 3, 5                       # image 3 has no valid descriptor; image 5 exactly one, in its last row block
PAIRS = [(i, j) for i in range(len(SIZES)) for j in range(len(SIZES)) if i != j] + [(7, 6)]   # 56 ordered pairs, one repeated
FAMILIES = ("random", "ties", "noisy")
OPTIONS = [(ratio, max_distance, cross_check) for ratio in (None, 0.8, 1.0) for max_distance in (0, 64, 256)
           for cross_check in (False, True)]
KIND_CYCLE = (go.KIND_ESSENTIAL, go.KIND_HOMOGRAPHY, go.KIND_NONE)
BANDS = ("narrow", "wide", "inf", "zero", "nan")    # per-pair thresholds: about 5 % admitted, about half, everything, ...
# per kind the motions its models cycle through: a pure rotation as an essential matrix is all zero and admits nothing
MOTION_NAMES = {go.KIND_ESSENTIAL: ("bench", "gen12_t", "pan10"), go.KIND_HOMOGRAPHY: ("pan10", "plane_bench", "gen12"),
                go.KIND_NONE: ("bench",)}
GEN12_T = np.array([-0.2, 0.4, 0.1])                # the translation of "gen12_t": gen12's rotation with a baseline


def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def motion_model(name, kind):
    """The essential matrix [t]x R of a motion of ``homography_oracle.MOTIONS`` (all zero for a pure rotation: every error is
    NaN and nothing is admitted), or the homography R + t n^T / d its plane z = 5 + 0.2 x - 0.1 y induces (R for a rotation)."""
    R, t, _ = ho.MOTIONS["gen12"] if name == "gen12_t" else ho.MOTIONS[name]
    t = GEN12_T if name == "gen12_t" else t
    if kind == go.KIND_ESSENTIAL:
        return skew(t) @ R
    z0, a, b = ho.PLANE
    return R + np.outer(t, np.array([-a, -b, 1.0])) / z0


def coordinates(sizes, seed):
    """Per image float64 (n, 2) K-normalised coordinates: feature f of an even image is point f of a seeded ``bench`` scene in
    its first view, of an odd image the same point in the second view; a random half is replaced by uniform coordinates in
    [-0.2, 0.2]^2."""
    rng = np.random.default_rng(seed)
    corr = ho.motion_scene("bench", max(max(sizes), 1), seed, 0.5)["corr"]
    out = []
    for k, n in enumerate(sizes):
        xy = corr[:n, :2].copy() if k % 2 == 0 else corr[:n, 2:].copy()
        uniform = rng.random(n) < 0.5
        xy[uniform] = rng.uniform(-0.2, 0.2, (int(uniform.sum()), 2))
        out.append(np.ascontiguousarray(xy))
    return out


def band_threshold(errors, band):
    """The threshold of a band for one pair's error matrix; the two quantiles are over its finite errors."""
    if band == "inf":
        return np.inf
    if band == "zero":
        return 0.0
    if band == "nan":
        return np.nan
    finite = errors[np.isfinite(errors)]
    if finite.size == 0:
        return 1.0
    return float(np.quantile(finite, 0.05 if band == "narrow" else 0.5))


@functools.lru_cache(maxsize=None)
def geometry():
    """What the three families share: (xy per image, models (Q, 3, 3), kinds (Q,) int32, thresholds (Q,), per pair the bool
    matrix ``err <= threshold``).  Prints each pair's admitted share."""
    xy = coordinates(SIZES, 7)
    Q = len(PAIRS)
    models, kinds, thresholds, within = np.zeros((Q, 3, 3)), np.zeros(Q, np.int32), np.zeros(Q), []
    for q, (i, j) in enumerate(PAIRS):
        # (the shift gives the pairs of the three large images with valid features, 4, 6 and 7, an essential matrix with the
        # wide and the narrow band, (6, 4) and (7, 6), and a homography with the wide one, the repeated (7, 6))
        kinds[q] = KIND_CYCLE[(q + 2) % 3]
        band = BANDS[q % 5]
        name = MOTION_NAMES[int(kinds[q])][(q // 3) % len(MOTION_NAMES[int(kinds[q])])]
        models[q] = motion_model(name, kinds[q] if kinds[q] else go.KIND_ESSENTIAL)
        if kinds[q] == go.KIND_NONE:
            thresholds[q] = band_threshold(np.zeros(0), band)
            within.append(np.zeros((SIZES[i], SIZES[j]), dtype=bool))
            continue
        e = go.errors(models[q], kinds[q], xy[i], xy[j])
        thresholds[q] = band_threshold(e, band)
        with np.errstate(invalid="ignore"):
            within.append(e <= thresholds[q])
        if e.size:
            print(f"pair {q} {PAIRS[q]} kind {kinds[q]} {name} {band}: threshold {thresholds[q]:.3e} admits "
                  f"{within[-1].mean():.3f}")
    return xy, models, kinds, thresholds, within


def descriptors(family, sizes=SIZES, seed=None):
    """(bits, valid) per image: the three families of tests/test_gpu_graph_matching.py."""
    rng = np.random.default_rng(FAMILIES.index(family) + 40 if seed is None else seed)
    pool = rng.integers(0, 256, (400, 32), dtype=np.uint8)
    three = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    images = []
    for k, n in enumerate(sizes):
        if family == "random":
            bits = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        elif family == "ties":
            bits = three[rng.integers(0, 3, n)]      # three values: ties for the best and the runner-up everywhere
        else:
            flips = np.zeros((n, 256), dtype=np.uint8)
            for row, count in zip(flips, rng.integers(0, 41, n)):   # a pool descriptor with 0 .. 40 flipped bits: real matches
                row[rng.choice(256, count, replace=False)] = 1
            bits = pool[rng.integers(0, len(pool), n)] ^ np.packbits(flips, axis=1, bitorder="little")
        images.append((bits, rng.random(n) < 0.9))   # scattered invalid features
    return images


class Collection:
    """One family on the shared geometry: ``images`` of (bits, valid, xy) and the oracle's summaries of PAIRS."""

    def __init__(self, family):
        xy, self.models, self.kinds, self.thresholds, within = geometry()
        self.images = []
        for k, (bits, valid) in enumerate(descriptors(family)):
            if k == ALL_INVALID:
                valid[:] = False
            if k == ONE_VALID:
                valid[:] = False
                valid[len(valid) - 1] = True
            bits.setflags(write=False)
            valid.setflags(write=False)
            self.images.append((bits, valid, xy[k]))
        matrices, self.per_pair = {}, []
        for q, (i, j) in enumerate(PAIRS):
            lo, hi = min(i, j), max(i, j)
            if (lo, hi) not in matrices:
                matrices[lo, hi] = gmo.distances(self.images[lo][0], self.images[hi][0])
            d = matrices[lo, hi] if i < j else matrices[lo, hi].T
            adm = within[q] & self.images[i][1][:, None] & self.images[j][1][None, :]
            self.per_pair.append(go.Summaries(d, adm))
        self.unguided = gmo.GraphSummaries([im[:2] for im in self.images], PAIRS)

    def decide(self, q, max_distance, ratio, cross_check):
        return gmo.decide(self.per_pair[q], max_distance, ratio, cross_check)

    def rows(self, max_distance=64, ratio=0.8, cross_check=True):
        out = [self.decide(q, max_distance, ratio, cross_check) for q in range(len(PAIRS))]
        return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])

    def matches(self, max_distance=64, ratio=0.8, cross_check=True):
        lists = [gmo.compact(*self.decide(q, max_distance, ratio, cross_check)) for q in range(len(PAIRS))]
        return [m for m, _ in lists], [d for _, d in lists]


@functools.lru_cache(maxsize=None)
def collection(family):
    """Computed once, shared by every test, never changed."""
    return Collection(family)


# ------------------------------------------------------------------------------------------------------
# the accuracy conditions: repeated structure, first pass against guided pass
# ------------------------------------------------------------------------------------------------------
THR = 6e-6
REPEATED = (4, 400, 250, 30, 80)   # views, points, unique, groups, extra


def relative_motion(poses, i, j):
    """(R, t) with x_j ~ R x_i + t from two rows of ``poses_true``."""
    Ri, ti, Rj, tj = poses[i, :9].reshape(3, 3), poses[i, 9:], poses[j, :9].reshape(3, 3), poses[j, 9:]
    R = Rj @ Ri.T
    return R, tj - R @ ti


def right_matches(matches, ids_a, ids_b):
    m = np.asarray(matches).reshape(-1, 2)
    return int(np.count_nonzero((ids_a[m[:, 0]] >= 0) & (ids_a[m[:, 0]] == ids_b[m[:, 1]])))


@functools.lru_cache(maxsize=None)
def repeated_chain(seed, ordered=True):
    """The NumPy chain on ``repeated_structure_views(*REPEATED, seed)`` with the true essential matrices at THR: dict(scene,
    images (bits, valid, xy), pairs, E (Q, 3, 3), first / guided: match lists per pair, rows: per pair (common, kept and right
    of the first pass, kept and right of the guided pass))."""
    from structure_from_motion_amd.feature_matching.guided_matching import essential_from_pose, normalized_coordinates

    sc = synthetic.repeated_structure_views(*REPEATED, seed)
    V = REPEATED[0]
    images = [(b, v, normalized_coordinates(sc["K"], p)) for (b, v), p in zip(sc["descriptors"], sc["pixels"])]
    pairs = [(i, j) for i in range(V) for j in range(V) if (i != j if ordered else i < j)]
    motions = [relative_motion(sc["poses_true"], i, j) for i, j in pairs]
    E = essential_from_pose(np.array([m[0] for m in motions]), np.array([m[1] for m in motions]))
    first, _ = gmo.match_graph([im[:2] for im in images], pairs)
    guided, _ = go.match_graph(images, pairs, E, [go.KIND_ESSENTIAL] * len(pairs), [THR] * len(pairs))
    rows = []
    for q, (i, j) in enumerate(pairs):
        ids_i, ids_j = sc["ids"][i], sc["ids"][j]
        common = len(set(ids_i[ids_i >= 0].tolist()) & set(ids_j[ids_j >= 0].tolist()))
        rows.append((common, len(first[q]), right_matches(first[q], ids_i, ids_j), len(guided[q]),
                     right_matches(guided[q], ids_i, ids_j)))
    return dict(scene=sc, images=images, pairs=np.array(pairs, dtype=np.int64), E=E, first=first, guided=guided, rows=rows)


# ------------------------------------------------------------------------------------------------------
# the stream case
# ------------------------------------------------------------------------------------------------------
@stream_cases.case(["sfm_match_pairs_guided"], [])
def match_pairs_guided(dev):
    """Six ordered pairs over images of 255 / 513 / 1030 features, essential and homography kinds with bands that admit about
    half, cross-check on: two scenes of equal shapes whose descriptors, flags and coordinates differ."""
    import torch

    from structure_from_motion_amd import device

    i = stream_cases.Inst(dev)
    sizes = (255, 513, 1030)
    pairs = np.array([(x, y) for x in range(3) for y in range(3) if x != y], dtype=np.int32)
    Q = len(pairs)
    kinds = np.array([KIND_CYCLE[q % 2] for q in range(Q)], dtype=np.int32)
    models = np.array([motion_model(("bench", "plane_bench")[q % 2], kinds[q]) for q in range(Q)])

    def scene(seed):
        images = descriptors("noisy", sizes, seed)
        return (np.concatenate([b for b, _ in images]), np.concatenate([v for _, v in images]).astype(np.uint8),
                np.concatenate(coordinates(sizes, seed)))
    a, b = scene(40), scene(41)
    thresholds = np.array([band_threshold(go.errors(models[q], kinds[q], coordinates(sizes, 40)[x], coordinates(sizes, 40)[y]), "wide")
                           for q, (x, y) in enumerate(pairs.tolist())])
    desc, ok, xy = i.inp(a[0], b[0]), i.inp(a[1], b[1]), i.inp(a[2], b[2])
    offset = np.zeros(4, dtype=np.int32)
    offset[1:] = np.cumsum(sizes)
    row_offset = np.zeros(Q + 1, dtype=np.int64)
    row_offset[1:] = np.cumsum(np.array(sizes)[pairs[:, 0]])
    rows, F = int(row_offset[-1]), int(sum(sizes))
    image_offset, pair_images, rows_dev = i.same(offset), i.same(pairs), i.same(row_offset)
    model_dev, kind_dev, thr_dev = i.same(models.reshape(Q, 9)), i.same(kinds), i.same(thresholds)
    partner, distance = i.out("partner", (rows,), torch.int32), i.out("distance", (rows,), torch.int32)
    status = i.out("pair_status", (Q,), torch.int32)
    i.constant.add("pair_status")
    ws = i.work(stream_cases._lib().sfm_match_pairs_workspace_bytes(Q, rows, 1030))
    i.call = lambda: device.match_pairs_guided(3, F, image_offset, desc, ok, xy, pair_images, rows_dev, model_dev, kind_dev,
                                               thr_dev, rows, 1030, 64, 0.8, True, partner, distance, status, workspace=ws)
    return i
