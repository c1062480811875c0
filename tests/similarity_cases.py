"""What the host and GPU tests of the similarity alignment share (tests/test_similarity_host.py, tests/test_gpu_similarity.py):
the fixtures, the measured tolerance, and the stream cases of the three entry points."""
import numpy as np

import similarity_oracle as so
import stream_cases
from geometry_cases import rotation

THR = 1e-6          # squared units of side B: a 1e-3 residual on clouds of unit extent
RMS = 3
SEED, STRIDE, H_BEGIN = 0x9E3779B97F4A7C15, 3, 5

# The oracle's two routes (SVD with the determinant correction, Horn's quaternion eigenvector) differ on the samples of the
# parity and special-motion fixtures below by at most 4.46e-13 in so.model_gap's measure (measured; tests/test_similarity_host.py
# prints it per fixture and bounds it by this constant).  The worst sample is the one closest to collinear, d / sqrt(sa2 sb2) =
# 5.8e-4 in entry 2 of fixture (3, 513, 257): the rotation about a nearly collinear triple is determined to about eps sigma_1 / d.  The
# device is held to ten times the gap.
ROUTE_GAP = 4.5e-13
PARITY_TOL = 10.0 * ROUTE_GAP
# samples this close to the degeneracy floor, on either side, are left out of the value comparison (never of the flags)
NEAR_BAND = 100.0
NEAR_CAP = 0.005    # at most this share of a fixture's hypotheses


def similarity(seed, scale=None):
    """A reproducible (s, R, t): rotation about a random axis by a random angle, scale in [0.5, 2) unless given."""
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=3)
    R = rotation(axis, rng.uniform(10.0, 160.0))
    return (float(rng.uniform(0.5, 2.0)) if scale is None else float(scale)), R, rng.uniform(-3.0, 3.0, size=3)


def pairs_of(a, sim, noise=0.0, seed=0):
    s, R, t = sim
    b = s * (a @ R.T) + t
    if noise:
        b = b + np.random.default_rng(seed + 7).normal(scale=noise, size=b.shape)
    return np.ascontiguousarray(np.hstack([a, b]))


def cloud(n, seed, extent=1.0, centre=0.0):
    return np.random.default_rng(seed).uniform(-extent, extent, size=(n, 3)) + centre


def scene(n, seed, outliers=0.0, noise=0.0, sim=None):
    """pairs (n, 6) of a cube cloud under `sim` (default: similarity(seed)); the first round(outliers n) shuffled positions get
    a side-B point displaced by 0.1 to 1.1 units (at least 100 x sqrt(THR)).  -> (pairs, sim, clean mask)."""
    sim = similarity(seed) if sim is None else sim
    pairs = pairs_of(cloud(n, seed), sim, noise, seed)
    clean = np.ones(n, dtype=bool)
    k = int(round(outliers * n))
    if k:
        rng = np.random.default_rng(seed + 1)
        bad = rng.permutation(n)[:k]
        direction = rng.normal(size=(k, 3))
        direction /= np.linalg.norm(direction, axis=1, keepdims=True)
        pairs[bad, 3:] += direction * rng.uniform(0.1, 1.1, size=(k, 1))
        clean[bad] = False
    return pairs, sim, clean


def batch_scene(batch, n, seed, **kw):
    """A different scene per entry: pairs (batch, n, 6), the truths and the clean masks."""
    scenes = [scene(n, seed + 100 * b, **kw) for b in range(batch)]
    return np.stack([s[0] for s in scenes]), [s[1] for s in scenes], np.stack([s[2] for s in scenes])


# (batch, n, h): 513 crosses the 512-item score tile, 257 the 256-lane score block and the 64-lane fit block
PARITY_SHAPES = [(1, 3, 1), (1, 4, 64), (3, 64, 257), (1, 513, 64), (3, 513, 257), (1, 64, 1)]


def parity_fixture(shape):
    """pairs (batch, n, 6) of one of PARITY_SHAPES: a different scene per entry, with noise of a third of sqrt(THR) per
    coordinate and 30 % displaced points, so that the counts and sums of the hypotheses differ."""
    batch, n, h = shape
    return batch_scene(batch, n, 40 + n + h, outliers=0.3, noise=3e-4)[0]


def half_turn(axis):
    return rotation(axis, 180.0)


def special_motions():
    """name -> pairs (64, 6), each of which must fit: the truth is the second entry."""
    a = cloud(64, 11)
    out = {"identity": (a, (1.0, np.eye(3), np.zeros(3)))}
    for name, axis in (("half_turn_x", (1, 0, 0)), ("half_turn_y", (0, 1, 0)), ("half_turn_z", (0, 0, 1)),
                       ("half_turn_skew", (1, -2, 3))):
        out[name] = (a, (1.3, half_turn(axis), np.array([0.5, -1.0, 2.0])))
    s, R, t = similarity(12)
    out["scale_1e-3"] = (a, (1e-3, R, t * 1e-3))
    out["scale_1e3"] = (a, (1e3, R, t * 1e3))
    out["far_from_origin"] = (cloud(64, 13, centre=1e6), (1.0, R, np.array([1e6, -1e6, 1e6]) - R @ np.full(3, 1e6) + np.full(3, 1e6)))
    flat = cloud(64, 14)
    flat[:, 2] = 0.25 * flat[:, 0] - 0.5 * flat[:, 1]   # a coplanar cloud
    out["coplanar"] = (flat, (s, R, t))
    return {k: (pairs_of(a_, sim), sim) for k, (a_, sim) in out.items()}


def mirror_pairs(n=64, seed=15):
    """B a mirror image of A: no proper rotation aligns more than a sample."""
    a = cloud(n, seed)
    s, R, t = similarity(seed)
    return np.ascontiguousarray(np.hstack([a, s * ((a * np.array([1.0, 1.0, -1.0])) @ R.T) + t]))


def near_degenerate(ratios):
    with np.errstate(invalid="ignore"):
        return (ratios > so.DEGENERATE_FLOOR / NEAR_BAND) & (ratios < so.DEGENERATE_FLOOR * NEAR_BAND)


def outlier_fixture():
    """The noise-free outlier case: 200 pairs, 30 % of side B displaced by at least 100 x sqrt(THR), h = 256, gate at half the
    clean count."""
    pairs, sim, clean = scene(200, 31, outliers=0.3)
    return pairs, sim, clean, 256, int(np.count_nonzero(clean)) // 2, 31


def reprojection_errors(poses, points, cam, pt, pixels, K):
    """Squared pixel errors of observations (camera cam[m], point pt[m]) under (m, 12) poses R | t."""
    R, t = poses[cam, :9].reshape(-1, 3, 3), poses[cam, 9:]
    c = np.einsum("mij,mj->mi", R, points[pt]) + t
    p = c @ K.T
    return np.sum((p[:, :2] / p[:, 2:3] - pixels) ** 2, axis=1)


# ---- the stream cases -----------------------------------------------------------------------------------------------------
# The op lists are empty on purpose, as for register_views (tests/register_views_cases.py): tests/test_stream_cases_host.py
# requires every op a case names to be in ops.FUNCTIONAL_OPS / INPLACE_OPS, two tuples that an earlier schema guard pins, and the
# ops of these calls are listed in ops.SIMILARITY_OPS.  The calls below still go through them, and their outputs are compared.
def _scene_pairs(batch, n, seed):
    return batch_scene(batch, n, seed, outliers=0.3, noise=1e-4)[0]


@stream_cases.case(["sfm_similarity_ransac_pass"], [])
def similarity_ransac_pass(dev):
    """``SimilarityWorkspace.run``: the in-place op on the test's buffers."""
    import torch

    from structure_from_motion_amd import device

    i = stream_cases.Inst(dev)
    # one spare stream of torch's pool beside the three cases of this module: four in all, so that every later side stream of
    # tests/test_gpu_streams.py keeps its hardware queue (the comment in tests/register_views_cases.py)
    i.keep_alignment = [torch.cuda.Stream()]
    B, n, h = 2, 700, 257
    pairs = i.inp(_scene_pairs(B, n, 3), _scene_pairs(B, n, 4))
    ws = device.SimilarityWorkspace(B, n, h, dev)
    ws.S, ws.model, ws.flags, ws.cnt, ws.s1, ws.s2, ws.result, ws.mask = stream_cases._pass_outputs(i, B, n, h, so.MODEL)
    i.call = lambda: ws.run(pairs, THR, 10, RMS, philox=(i.cur, 100, 3))
    return i


@stream_cases.case(["sfm_similarity_fit_masked"], [])
def similarity_fit_masked(dev):
    """5000 items (three blocks of partial sums) through the C ABI on the test's workspace, with a mask and without; the
    functional op on the same inputs (outputs only)."""
    import torch

    from structure_from_motion_amd import device

    i = stream_cases.Inst(dev)
    B, n = 2, 5000
    (pa, _, ca), (pb, _, cb) = batch_scene(B, n, 5, outliers=0.3), batch_scene(B, n, 6, outliers=0.3)
    pairs, mask = i.inp(pa, pb), i.inp(ca.astype(np.uint8), cb.astype(np.uint8))
    model, flags = i.out("model", (B, so.MODEL), torch.float64), i.out("flags", (B,), torch.int32)
    model_all, flags_all = i.out("model_all", (B, so.MODEL), torch.float64), i.out("flags_all", (B,), torch.int32)
    i.constant |= {"flags", "flags_all"}
    lib = stream_cases._lib()
    ws = i.work(lib.sfm_similarity_fit_workspace_bytes(n, B))

    def call():
        stream_cases._check(lib.sfm_similarity_fit_masked(pairs.data_ptr(), n, B, mask.data_ptr(), model.data_ptr(), flags.data_ptr(),
                                                          ws.data_ptr(), ws.numel(), stream_cases._st()), "sfm_similarity_fit_masked")
        stream_cases._check(lib.sfm_similarity_fit_masked(pairs.data_ptr(), n, B, None, model_all.data_ptr(), flags_all.data_ptr(),
                                                          ws.data_ptr(), ws.numel(), stream_cases._st()), "sfm_similarity_fit_masked")
        return stream_cases.Returned([device.fit_similarity(pairs, mask)[0]])   # (its flags are all zero in both scenes)
    i.call = call
    return i


@stream_cases.case(["sfm_similarity_refine"], [])
def similarity_refine(dev):
    """rounds = 3 through the C ABI on the test's buffers and workspace, and through the functional op (outputs only)."""
    import torch

    from structure_from_motion_amd import device

    i = stream_cases.Inst(dev)
    B, n, h = 2, 5000, 64

    def finished(seed):
        pairs = torch.as_tensor(_scene_pairs(B, n, seed)).to(dev)
        ws = device.SimilarityWorkspace(B, n, h, dev)
        ws.run(pairs, THR, 10, RMS, philox=(9, 100, 3))
        torch.cuda.synchronize()
        return (pairs,) + stream_cases._winner(ws) + (ws.mask,)
    a, b = finished(3), finished(4)
    pairs, model, err, mask = (i.inp(x, y) for x, y in zip(a, b))
    model_out, mask_out = i.out("model_out", (B, so.MODEL), torch.float64), i.out("mask_out", (B, n), torch.uint8)
    info = i.out("info", (B, 3), torch.int64)
    lib = stream_cases._lib()
    ws = i.work(lib.sfm_similarity_refine_workspace_bytes(n, B))

    def call():
        stream_cases._check(lib.sfm_similarity_refine(pairs.data_ptr(), n, B, model.data_ptr(), mask.data_ptr(), err.data_ptr(), THR,
                                                      RMS, 3, model_out.data_ptr(), mask_out.data_ptr(), info.data_ptr(), ws.data_ptr(),
                                                      ws.numel(), stream_cases._st()), "sfm_similarity_refine")
        return stream_cases.Returned(device.similarity_refine(pairs, model, mask, err, THR, RMS, rounds=3))
    i.call = call
    return i
