"""Fixtures and the stream case of the pair-pose refinement (sfm_refine_pair_poses).

``fixture`` is the hand-built call of the parity tests: every segment length at which the kernel takes another path, a pair
without a pose between pairs with one, and the special pairs of the issue.  ``accuracy_graph`` is the twelve-pair match graph
of the feature test and ``oracle_chain`` the NumPy route to its start poses.

Importing this module registers the stream case of the new entry point in ``stream_cases.CASES``; the two test files of the
feature import it at their top and sort before test_gpu_streams.py and test_stream_cases_host.py, so both of those see the
complete table in a run of the whole suite."""
import functools

import numpy as np

import homography_oracle as ho
import pair_refine_oracle as pr
import stream_cases
import view_graph_oracle as vo
import view_graph_pose_oracle as po
from geometry_cases import rotation
from oracle import sfm_oracle as orc

THR = 6e-6
POSE_DTYPE = np.dtype([("R", "<f8", (3, 3)), ("t", "<f8", (3,)), ("median_angle", "<f8"), ("votes", "<i4", (4,)), ("best", "<i4"),
                       ("status", "<i4")])

# (rounds, max_steps, aggregation, compared pairs) of the device-against-oracle comparisons: both round counts, one, two and
# four steps, each aggregation once.  A parity case needs every accept test and every threshold test decided well above
# rounding, or the device and the oracle may rightly part there (test_pair_refine_host.py checks both margins on every
# compared pair of every run).  These starts are 0.05 degrees from the truth and Gauss-Newton with lambda = 1e-3 gains three
# to four digits a step, so the third trial of a noisy pair lowers the cost by 1e-8 of it or less and the fourth by 1e-13: a
# run of four steps is compared on the pairs whose steps stay decided (six items: a slow start; the forward motion: one weak
# direction) and on the pairs that take no step; a second round restarts converged and is compared with one step.
FOUR_STEP_NAMES = ("empty", "five", "six", "no_model", "true_pose", "repeated", "tz")
PARITY_RUNS = ((2, 1, pr.RMS, None), (1, 2, pr.SUM, None), (2, 1, pr.SQUARE, None), (1, 1, pr.MEAN, None),
               (2, 4, pr.RMS, FOUR_STEP_NAMES))
MIN_ACCEPT_MARGIN = 1e-10
MIN_THRESHOLD_MARGIN = 1e-6
# The largest difference between two runs of the oracle over the fixture and PARITY_RUNS, items in the given order and
# reversed (test_pair_refine_host.py re-measures it): the absolute difference of R and t, the relative one of both errors.
# The device is allowed ten times as much.
# Measured over the compared pairs: R 1.25e-15, t 3.77e-15, errors 8.34e-14 (the six-item pair, whose error is 1e-4 of the
# threshold, carries all three); rounded up.
SPREAD = dict(R=1.3e-15, t=3.8e-15, error=8.4e-14)
DEVICE_TOLERANCE = {k: 10.0 * v for k, v in SPREAD.items()}


def perturbed(R, t, degrees, seed):
    """(R, t) moved by a rotation of ``degrees`` about a random axis, the unit t by as much about another."""
    rng = np.random.default_rng(seed)
    t = t / np.linalg.norm(t)
    return rotation(rng.normal(size=3), degrees) @ R, rotation(rng.normal(size=3), degrees) @ t


def _record(R, t, status=po.OK):
    rec = np.zeros((), dtype=POSE_DTYPE)
    rec["R"], rec["t"], rec["status"] = R, t, status
    rec["median_angle"], rec["votes"], rec["best"] = 0.05, (7, 0, 3, 1), 0   # carried over byte for byte
    if status != po.OK:
        rec["R"], rec["t"], rec["median_angle"], rec["votes"], rec["best"] = np.nan, np.nan, np.nan, 0, -1
    return rec


NAMES = ("empty", "five", "six", "n255", "no_model", "n256", "n257", "n1025", "true_pose", "repeated", "nan_item", "tz", "pan")
TZ_MOTION = (rotation((0.3, 1.0, -0.2), 4.0), np.array([0.0, 0.0, 1.0]))


@functools.lru_cache(maxsize=None)
def fixture(seed=0):
    """(corr (N, 4), offset (Q + 1,), pose table (Q,) of POSE_DTYPE), pairs in the order of NAMES:
    segments of 0, 5, 6, 255, 256, 257 and 1025 items (both sides of the block stride of 256, and four strides plus one), a
    pair whose pose status is not OK between them, a noise-free pair at its true pose, one correspondence 300 times, a pair
    with a NaN item, a forward motion started at t = (0, 0, 1) exactly (the tie of the basis rule) and a pure pan with a pose.
    The noisy pairs have 0.5 px noise and 30 % outliers and start 0.05 degrees from the truth."""
    bench, gen = po.MOTIONS["bench"][:2], po.MOTIONS["gen12_t"][:2]
    parts, poses = [], []

    def add(corr, R, t, status=po.OK):
        parts.append(np.ascontiguousarray(corr, dtype=np.float64).reshape(-1, 4))
        poses.append(_record(R, t, status))

    def noisy(motion, n, k, outliers=0.3):
        return ho.scene(motion[0], motion[1], False, n, seed + 10 * k, 0.5, outliers)["corr"]

    add(np.zeros((0, 4)), *perturbed(*bench, 0.05, seed + 1))
    add(noisy(bench, 5, 1, 0.0), *perturbed(*bench, 0.05, seed + 2))
    add(noisy(bench, 6, 2, 0.0), *perturbed(*bench, 0.05, seed + 3))
    add(noisy(bench, 255, 3), *perturbed(*bench, 0.05, seed + 4))
    add(noisy(bench, 40, 4), np.eye(3), np.zeros(3), po.NO_MODEL)
    add(noisy(gen, 256, 5), *perturbed(*gen, 0.05, seed + 5))
    add(noisy(bench, 257, 6), *perturbed(*bench, 0.05, seed + 6))
    add(noisy(gen, 1025, 7), *perturbed(*gen, 0.05, seed + 7))
    add(ho.scene(*bench, False, 100, seed + 80)["corr"], bench[0], bench[1] / np.linalg.norm(bench[1]))
    add(np.repeat(ho.scene(*bench, False, 1, seed + 90, 0.5)["corr"], 300, axis=0), *perturbed(*bench, 0.02, seed + 8))
    with_nan = noisy(bench, 120, 10).copy()
    with_nan[7, 0] = np.nan
    add(with_nan, *perturbed(*bench, 0.05, seed + 9))
    add(noisy(TZ_MOTION, 200, 11), perturbed(*TZ_MOTION, 0.05, seed + 10)[0], TZ_MOTION[1])
    pan = po.MOTIONS["pan10"][0]
    add(noisy((pan, np.zeros(3)), 150, 12), perturbed(pan, np.array([1.0, 0.0, 0.0]), 0.05, seed + 11)[0], np.array([1.0, 0.0, 0.0]))
    assert len(parts) == len(NAMES)
    offset = np.zeros(len(parts) + 1, dtype=np.int64)
    offset[1:] = np.cumsum([len(p) for p in parts])
    return np.ascontiguousarray(np.concatenate(parts)), offset, np.array(poses)


def pose_dicts(table):
    """A POSE_DTYPE table as the list of dicts ``pair_refine_oracle.refine_pairs`` takes."""
    return [dict(status=int(r["status"]), R=r["R"].copy(), t=r["t"].copy()) for r in table]


@functools.lru_cache(maxsize=None)
def compared(names):
    """The pair indices a run is compared on."""
    return [q for q, name in enumerate(NAMES) if names is None or name in names]


@functools.lru_cache(maxsize=None)
def oracle_runs(seed=0):
    """{(rounds, max_steps, aggregation): (results, mask, reversed results, traces)} of the fixture under PARITY_RUNS."""
    corr, offset, table = fixture(seed)
    out = {}
    for rounds, steps, agg, _ in PARITY_RUNS:
        traces = {}
        res, mask = pr.refine_pairs(corr, offset, pose_dicts(table), THR, agg, rounds, steps, traces=traces)
        rev, mask_rev = pr.refine_pairs(corr, offset, pose_dicts(table), THR, agg, rounds, steps, reverse=True)
        assert np.array_equal(mask, mask_rev)
        out[(rounds, steps, agg)] = (res, mask, rev, traces)
    return out


# ------------------------------------------------------------------------------------------------------
# the accuracy condition: twelve pairs, `bench` and `gen12_t`, 300 matches, 0.5 px, 30 % outliers, scene seeds 0-5
# ------------------------------------------------------------------------------------------------------
ACCURACY_MOTIONS = ("bench", "gen12_t")
ACCURACY_SEED = 1000       # pair q draws its samples with ACCURACY_SEED + q
ACCURACY_ITERATIONS = 256
ACCURACY_GATE = 20         # 300 // 15, the gate of the view-graph fixture: without one the lowest RMS wins on a handful of items
MAX_WORSE = 4


@functools.lru_cache(maxsize=None)
def accuracy_scenes():
    return tuple(po.motion_scene(name, 300, s, 0.5, 0.3) for name in ACCURACY_MOTIONS for s in range(6))


def accuracy_graph():
    """(features, pairs, matches) of the twelve scenes in ``verify_pairs``'s formats."""
    return vo.match_graph(list(accuracy_scenes()))


def oracle_chain(sc, seed, iterations=ACCURACY_ITERATIONS, thr=THR, gate=ACCURACY_GATE):
    """The start pose of one pair by NumPy alone: ``five_point.fit_corr`` on the Philox samples of ``seed``, six-item scoring
    and the selection rule of view_graph_oracle, the winner's mask and the pose oracle -> its dict."""
    from structure_from_motion_amd.epipolar import five_point as fp

    corr = sc["corr"]
    n = len(corr)
    S = orc.philox_sample_table(seed, 0, iterations, n)
    E, flags = fp.fit_corr(corr, S)
    cnt, s1, s2 = np.zeros(iterations, np.int64), np.full(iterations, np.nan), np.full(iterations, np.nan)
    for k in range(iterations):
        if flags[k] or not np.isfinite(E[k]).all():
            continue
        with np.errstate(all="ignore"):
            e = orc.sed_values(E[k].reshape(3, 3), corr)
        rest = np.ones(n, bool)
        rest[S[k, :6]] = False
        inl = rest & (e <= thr)
        cnt[k] = inl.sum()
        s1[k] = e[S[k, :6]].sum() + e[inl].sum()
        s2[k] = (e[S[k, :6]] ** 2).sum() + (e[inl] ** 2).sum()
    best, _ = vo.select(cnt, s1, s2, flags, gate, vo.E_SAMPLE)
    assert best >= 0
    return po.pair_pose(corr, vo.essential_mask(corr, E, S, best, thr), E[best].reshape(3, 3))


def pose_errors(R, t, scenes):
    """(Q, 2): rotation error and translation-direction error in degrees against each scene's truth."""
    return np.array([[pr.rotation_error_deg(R[q], sc["R"]), pr.direction_error_deg(t[q], sc["t"])] for q, sc in enumerate(scenes)])


def accuracy_summary(before, after):
    """dict(median_before (2,), median_after (2,), worse: pairs worse in either measure)."""
    return dict(median_before=np.median(before, axis=0), median_after=np.median(after, axis=0),
                worse=int(np.count_nonzero((after > before).any(axis=1))))


# ------------------------------------------------------------------------------------------------------
# the stream case
# ------------------------------------------------------------------------------------------------------
# The op list is empty on purpose: tests/test_stream_cases_host.py requires every op a case names to be in ops.FUNCTIONAL_OPS /
# INPLACE_OPS, and refine_pair_poses is listed in ops.LATER_FUNCTIONAL_OPS (the first two are pinned by an earlier schema
# guard).  The call below still goes through the op, and its outputs are compared.
@stream_cases.case(["sfm_refine_pair_poses"], [])
def refine_pair_poses(dev):
    """The fixture on two seeds, two rounds of four steps: through the C ABI on the test's buffers, and through the
    functional op (outputs only)."""
    import torch

    from structure_from_motion_amd import device

    i = stream_cases.Inst(dev)
    a, b = fixture(0), fixture(100)
    assert np.array_equal(a[1], b[1])
    N, Q = len(a[0]), len(a[2])
    corr = i.inp(a[0], b[0])
    pose = i.inp(a[2].view(np.uint8).reshape(Q, 128), b[2].view(np.uint8).reshape(Q, 128))
    offset = i.same(a[1], torch.int64)
    pose_out, mask = i.out("pose_out", (Q, 128), torch.uint8), i.out("mask", (N,), torch.uint8)
    info = i.out("info", (Q, 5), torch.int64)
    lib = stream_cases._lib()

    def call():
        stream_cases._check(lib.sfm_refine_pair_poses(corr.data_ptr(), N, offset.data_ptr(), Q, pose.data_ptr(), THR, pr.RMS, 2, 4,
                                                      pose_out.data_ptr(), mask.data_ptr(), info.data_ptr(), stream_cases._st()),
                            "sfm_refine_pair_poses")
        return stream_cases.Returned(device.refine_pair_poses(corr, offset, pose, THR, pr.RMS, rounds=2, max_steps=4))
    i.call = call
    return i
