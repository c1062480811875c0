"""Helpers of the view-graph tests: the ragged fixture, the definitions a call is checked against (selection,
masks, verdict — the NumPy definitions of tests/homography_oracle.py and oracle/sfm_oracle.py with the sample size as a
parameter), and match graphs built from two-view scenes.  Imported by tests/test_view_graph_host.py and
tests/test_gpu_view_graph.py."""
import numpy as np

import homography_oracle as ho
from oracle import sfm_oracle as orc

THR = 2e-5
RMS = 3
H_SAMPLE, E_SAMPLE = 4, 6
NONE, ESSENTIAL, HOMOGRAPHY, BAD_OFFSETS = range(4)
# both sample sizes, both sides of the 512-item tile of the scoring kernel, and two tiles plus one
SIZES = (0, 3, 4, 5, 6, 7, 8, 300, 511, 512, 513, 1025)
MOTION_CYCLE = ("bench", "pan10", "plane_bench", "gen12")


# a second fixture on the special motions and planes of tests/homography_cases.py: the sizes cycle both sample sizes and both
# sides of the 64-lane block; the pairs of 300 and 513 items are scenes that one homography explains, so both models exist
SPECIAL_SIZES = (6, 7, 64, 65, 300, 513) * 2
SPECIAL_SCENES = (("roll180_tx", "general"), ("turn170", "plane"), ("tz", "general"), ("roll15_tz", "general"), ("tz", "fronto"),
                  ("tx", "steep"), ("roll90_tgen", "steep"), ("ty", "fronto"), ("gen_tz", "plane"), ("roll180", "general"),
                  ("still", "general"), ("roll90", "general"))


def ragged_scenes(sizes=SIZES, seed=40, scenes=None):
    """One scene per size, 30 % outliers and 0.5 px noise: cycling the four motions, or (``scenes``) the (motion, shape) pairs
    of homography_cases in turn."""
    if scenes is None:
        return [ho.motion_scene(MOTION_CYCLE[k % 4], n, seed + k, 0.5, 0.3) for k, n in enumerate(sizes)]
    import homography_cases as hc

    return [hc.scene(*scenes[k % len(scenes)], n, seed + k, 0.5, 0.3) for k, n in enumerate(sizes)]


def ragged_arrays(scenes):
    """(corr (N, 4), offset int64 (Q + 1,), min_extra (Q,) = n_q // 15)."""
    counts = np.array([len(sc["corr"]) for sc in scenes], dtype=np.int64)
    offset = np.zeros(len(scenes) + 1, dtype=np.int64)
    offset[1:] = np.cumsum(counts)
    corr = np.concatenate([sc["corr"].reshape(-1, 4) for sc in scenes])
    return np.ascontiguousarray(corr), offset, (counts // 15).astype(np.float64)


def match_graph(scenes):
    """(features, pairs, matches) in build_tracks's formats: scene q is images 2q and 2q + 1, matched item by item."""
    features, pairs, matches = [], [], []
    for q, sc in enumerate(scenes):
        features += [sc["pix_a"].reshape(-1, 2), sc["pix_b"].reshape(-1, 2)]
        pairs.append((2 * q, 2 * q + 1))
        k = np.arange(len(sc["pix_a"]), dtype=np.int64)
        matches.append(np.column_stack([k, k]))
    return features, np.array(pairs, dtype=np.int64), matches


def select(cnt, s1, s2, flags, min_extra, sample, method=RMS):
    """homography_oracle.select with ``sample`` items per sample: (best index or -1, its error or inf)."""
    if sample == ho.SAMPLE:
        return ho.select(cnt, s1, s2, flags, min_extra, method)
    nn = cnt.astype(np.float64) + float(sample)
    with np.errstate(all="ignore"):
        err = [s1, s2, s1 / nn, np.sqrt(s2 / nn)][method]
        ok = (cnt >= min_extra) & (err < np.inf) & (flags == 0)
    if not ok.any():
        return -1, np.inf
    best = int(np.argmin(np.where(ok, err, np.inf)))
    return best, float(err[best])


def essential_mask(corr, E, S, best, thr):
    """uint8 (n,): 2 for the six sample items of hypothesis ``best``, 1 other items with sed <= thr, 0 otherwise; all zero for
    best < 0."""
    out = np.zeros(corr.shape[0], dtype=np.uint8)
    if best < 0:
        return out
    with np.errstate(invalid="ignore"):
        out[orc.sed_values(E[best].reshape(3, 3), corr) <= thr] = 1
    out[S[best, :E_SAMPLE]] = 2
    return out


def verdict(h_best, h_cnt, e_best, e_cnt, max_ratio):
    """(kind, homography count, essential count, ratio) from the two winners and their extra-inlier counts."""
    hc = H_SAMPLE + h_cnt if h_best >= 0 else 0
    ec = E_SAMPLE + e_cnt if e_best >= 0 else 0
    ratio = hc / ec if ec else float("inf")
    kind = NONE if hc == 0 and ec == 0 else (HOMOGRAPHY if ec == 0 or ratio > max_ratio else ESSENTIAL)
    return kind, hc, ec, ratio
