"""NumPy definition of the multi-scale FAST keypoints with BRIEF per pyramid level.

Everything is integer arithmetic on uint8 images widened to int64, so the HIP kernels (csrc/sfm_keypoints.hip) are compared byte
for byte.

  pyramid      level 0 is the image; level l + 1 is (4H // 5, 4W // 5) and exists iff l + 1 < levels and both sides are >= 48.
               Pixel (x', y') samples level l at ux = 10 x' + 1, x0 = ux >> 3, fx = ux & 7 (the same in y):
               ((8-fy)((8-fx) I[y0,x0] + fx I[y0,x0+1]) + fy((8-fx) I[y0+1,x0] + fx I[y0+1,x0+1]) + 32) >> 6
  FAST-9       circle pixel k is brighter iff I_k > p + t, darker iff I_k < p - t; a corner has 9 cyclically contiguous
               brighter or darker pixels; score = max(sum_brighter (I_k - p - t), sum_darker (p - I_k - t)); only centres with
               15 <= x <= W - 16 and 15 <= y <= H - 16 are tested, every other pixel scores 0
  suppression  on the unsuppressed map: p survives iff score(p) > 0, score(p) > score(n) for the neighbours n before p in raster
               order and score(p) >= score(n) for those after it; outside the plane scores 0
  quota        w_l = 4^l 5^(L-1-l); quota_l = N w_l // sum w; the remainder goes to level 0
  order        level ascending, then (score descending, y ascending, x ascending); a level keeps its first quota_l
  position     x_0 = 1.25^l (x_l + 0.5) - 0.5
  descriptor   tests/brief_oracle.describe(plane_l, [(x_l, y_l)])
"""
import numpy as np

import brief_oracle

CIRCLE = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3),
          (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3))
BORDER, MIN_SIDE, MAX_LEVELS, ARC = 15, 48, 12, 9


def next_shape(height: int, width: int):
    return 4 * height // 5, 4 * width // 5


def level_shapes(height: int, width: int, levels: int):
    """[(H_l, W_l)] of the levels an image of this size has."""
    shapes = [(int(height), int(width))]
    while len(shapes) < levels:
        h, w = next_shape(*shapes[-1])
        if h < MIN_SIDE or w < MIN_SIDE:
            break
        shapes.append((h, w))
    return shapes


def downsample(plane: np.ndarray) -> np.ndarray:
    """The next level of a uint8 plane."""
    I = plane.astype(np.int64)
    h, w = next_shape(*plane.shape)
    uy, ux = 10 * np.arange(h, dtype=np.int64) + 1, 10 * np.arange(w, dtype=np.int64) + 1
    y0, fy = (uy >> 3)[:, None], (uy & 7)[:, None]
    x0, fx = (ux >> 3)[None, :], (ux & 7)[None, :]
    top = (8 - fx) * I[y0, x0] + fx * I[y0, x0 + 1]
    bottom = (8 - fx) * I[y0 + 1, x0] + fx * I[y0 + 1, x0 + 1]
    return (((8 - fy) * top + fy * bottom + 32) >> 6).astype(np.uint8)


def pyramid(image: np.ndarray, levels: int):
    """The planes of an image: a list of uint8 arrays, level 0 first."""
    image = np.asarray(image)
    assert image.ndim == 2 and image.dtype == np.uint8 and 1 <= levels <= MAX_LEVELS
    planes = [image]
    for _ in level_shapes(*image.shape, levels)[1:]:
        planes.append(downsample(planes[-1]))
    return planes


def fast_scores(plane: np.ndarray, threshold: int) -> np.ndarray:
    """uint16 [H, W]: the FAST-9 score of every pixel, 0 where there is no corner or no test."""
    H, W = plane.shape
    out = np.zeros((H, W), dtype=np.uint16)
    h, w = H - 2 * BORDER, W - 2 * BORDER
    if h <= 0 or w <= 0:
        return out
    I = plane.astype(np.int64)
    p = I[BORDER:H - BORDER, BORDER:W - BORDER]
    ring = np.stack([I[BORDER + dy:BORDER + dy + h, BORDER + dx:BORDER + dx + w] for dx, dy in CIRCLE])
    brighter, darker = ring > p + threshold, ring < p - threshold

    def arc(mask):
        found = np.zeros(p.shape, dtype=bool)
        for start in range(16):
            run = np.ones(p.shape, dtype=bool)
            for k in range(ARC):
                run &= mask[(start + k) % 16]
            found |= run
        return found

    corner = arc(brighter) | arc(darker)
    strength = np.maximum(np.sum(np.where(brighter, ring - p - threshold, 0), axis=0),
                          np.sum(np.where(darker, p - ring - threshold, 0), axis=0))
    out[BORDER:H - BORDER, BORDER:W - BORDER] = np.where(corner, strength, 0)
    return out


def suppress(score: np.ndarray) -> np.ndarray:
    """uint16 [H, W]: the score of every survivor of the 3 x 3 suppression, 0 elsewhere."""
    H, W = score.shape
    s = score.astype(np.int64)
    padded = np.zeros((H + 2, W + 2), dtype=np.int64)
    padded[1:-1, 1:-1] = s
    keep = s > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            n = padded[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
            keep &= (s > n) if (dy < 0 or (dy == 0 and dx < 0)) else (s >= n)
    return np.where(keep, s, 0).astype(np.uint16)


def quotas(num_levels: int, num_features: int):
    """[quota_l] of an image with this many levels, in exact integers."""
    weights = [4 ** l * 5 ** (num_levels - 1 - l) for l in range(num_levels)]
    total = sum(weights)
    q = [int(num_features) * w // total for w in weights]
    q[0] += int(num_features) - sum(q)
    return q


def ordered_survivors(kept: np.ndarray):
    """(x, y, score) int64 arrays of a suppressed map's survivors by (score descending, y ascending, x ascending)."""
    y, x = np.nonzero(kept)
    s = kept[y, x].astype(np.int64)
    order = np.lexsort((x, y, -s))
    return x[order].astype(np.int64), y[order].astype(np.int64), s[order]


def base_xy(x, y, level):
    """Level pixels -> base-image pixels, float64 [n, 2]."""
    scale = np.float64(1.25) ** np.asarray(level, dtype=np.float64)
    return np.column_stack([scale * (np.asarray(x, dtype=np.float64) + 0.5) - 0.5,
                            scale * (np.asarray(y, dtype=np.float64) + 0.5) - 0.5]).reshape(-1, 2)


class Maps:
    """Everything about one image that ``num_features`` does not touch: planes, score maps and ordered survivors per level."""

    def __init__(self, image, levels: int, threshold: int):
        assert 1 <= threshold <= 254
        self.planes = pyramid(image, levels)
        self.scores = [fast_scores(p, threshold) for p in self.planes]
        self.kept = [suppress(s) for s in self.scores]
        self.survivors = [ordered_survivors(k) for k in self.kept]

    def select(self, num_features: int, levels=None):
        """(level_x, level_y, level, score) int64 arrays of the image's keypoints, in the definition's order.  ``levels``: as if
        the pyramid had been built with that smaller ``levels`` (the planes of a pyramid do not depend on those above them)."""
        count = len(self.planes) if levels is None else min(int(levels), len(self.planes))
        xs, ys, ls, ss = [], [], [], []
        for l, (quota, (x, y, s)) in enumerate(zip(quotas(count, num_features), self.survivors)):
            xs.append(x[:quota])
            ys.append(y[:quota])
            ss.append(s[:quota])
            ls.append(np.full(len(x[:quota]), l, dtype=np.int64))
        return np.concatenate(xs), np.concatenate(ys), np.concatenate(ls), np.concatenate(ss)


class Keypoints:
    def __init__(self, xy, level, score, bits, valid, angle_bin, level_xy):
        self.xy, self.level, self.score = xy, level, score
        self.bits, self.valid, self.angle_bin = bits, valid, angle_bin
        self.level_xy = level_xy                       # int64 [n, 2]: (x_l, y_l) on the keypoint's own plane


def describe(maps: Maps, num_features: int, memo=None, levels=None) -> Keypoints:
    """The keypoints of one image with their descriptors.  ``memo`` (a dict, optional) remembers descriptors per
    (level, x, y) of this image's planes across calls; ``levels``: see ``Maps.select``."""
    x, y, level, score = maps.select(num_features, levels)
    n = len(x)
    bits, valid, bins = np.zeros((n, 32), np.uint8), np.zeros(n, bool), np.zeros(n, np.uint8)
    for i in range(n):
        key = (int(level[i]), int(x[i]), int(y[i]))
        if memo is None or key not in memo:
            b, v, a = brief_oracle.describe(maps.planes[key[0]], np.array([[key[1], key[2]]], dtype=np.float64))
            entry = (b[0], bool(v[0]), int(a[0]))
            if memo is not None:
                memo[key] = entry
        else:
            entry = memo[key]
        bits[i], valid[i], bins[i] = entry
    return Keypoints(base_xy(x, y, level), level.astype(np.uint8), score.astype(np.int32), bits, valid, bins,
                     np.column_stack([x, y]).astype(np.int64).reshape(-1, 2))


def detect_and_describe(images, num_features=1000, levels=8, threshold=20):
    """The definition of ``feature_matching.keypoints.detect_and_describe``: one ``Keypoints`` per image."""
    return [describe(Maps(image, levels, threshold), num_features) for image in images]
