"""The three batched entry points of the pose stage called directly through the C ABI, at the sizes where the chunk compaction
of csrc/sfm_cheirality.h can go wrong: the edges of a wave (64), of a chunk (512) and of a four-wave block (2048).

``sfm_cheirality_batched`` is held to ``sfm_cheirality`` and to the oracle on DECISIONS, not on points: the two kernels put
different items in a wave, and the last bits of a DLT solve depend on a lane's wave-mates.  That is only safe away from the
thresholds, so every item compared is first shown, on the CPU, to keep a margin: the oracle's X[2] and z2 at least 1e-6 away
from -1e-8 and its norm at least 1e-6 (relative) away from the distance threshold.  The scenes are inlier-only
(``synthetic_two_view(outlier_fraction=0)``, seeds chosen on the CPU so that the margin holds for every item, pose and table);
outliers come in through the masks."""
import ctypes as C

import numpy as np
import pytest

from oracle import sfm_oracle as orc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_VALUES = (1, 63, 64, 65, 511, 512, 513, 2048, 2049)
N_MAX = max(N_VALUES)
CHUNK = 512
SEEDS = (11, 12)          # pair 0: the scene as it is; pair 1: another scene with its views swapped (the inverse motion)
THRESHOLD = 10.0          # in baselines: about half of the points of either scene lie beyond it, so decisions differ item by item
MARGIN = 1e-6
MASKS = ("ones", "zeros", "none", "random35", "one_in_last_chunk", "chunk_of_64", "chunk_of_65")


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def scenes():
    """Per pair: pixels of both views, K, the normalised correspondences [N_MAX, 4] and the essential matrix of the motion."""
    out = []
    for b, seed in enumerate(SEEDS):
        pa, pb, K, R, t, _ = orc.synthetic_two_view(N_MAX, seed=seed, outlier_fraction=0.0)
        if b == 1:
            pa, pb, R, t = pb, pa, R.T, -R.T @ t
        corr = orc.pack_correspondences(orc.to_normalized_image_coords(pa, K), orc.to_normalized_image_coords(pb, K))
        out.append(dict(pa=pa, pb=pb, K=K, corr=corr, E=skew(t / np.linalg.norm(t)) @ R))
    return out


def perturbed(table):
    """The table with the t of candidates 1 and 3 of each pair one bit off the negation of candidates 0 and 2: no antipodal pair
    is left, so every pose is solved on its own."""
    out = table.copy()
    out[:, 1::2, 11] = np.nextafter(out[:, 1::2, 11], np.inf)
    assert not np.array_equal(out[:, 1::2, 9:], -out[:, 0::2, 9:])
    return out


def assert_margins(corr, table):
    """Every item of ``corr`` [n, 4] under every pose of ``table`` [4, 12] is at least MARGIN away from each threshold of the test
    (oracle values).  Returns the oracle's decisions [4, n]."""
    want = np.empty((4, corr.shape[0]), dtype=bool)
    for p in range(4):
        R, t = table[p, :9].reshape(3, 3), table[p, 9:]
        P2 = np.eye(4)
        P2[:3, :3], P2[:3, 3] = R, t
        X = orc.triangulate_dlt(corr, np.eye(4), P2)
        z2 = (np.hstack([X, np.ones((len(X), 1))]) @ P2.T)[:, 2]
        norm = np.sqrt((X * X).sum(axis=1))
        assert np.all(np.isfinite(X))
        assert np.min(np.abs(X[:, 2] + orc.CHEIRALITY_TOLERANCE)) >= MARGIN, (p, "X[2]")
        assert np.min(np.abs(z2 + orc.CHEIRALITY_TOLERANCE)) >= MARGIN, (p, "z2")
        assert np.min(np.abs(norm - THRESHOLD)) >= MARGIN * THRESHOLD, (p, "norm")
        want[p] = orc.cheirality_pass(corr, R, t, THRESHOLD)
    return want


def make_mask(kind, n, seed):
    """[2, n] uint8, or None."""
    if kind == "none":
        return None
    rng = np.random.default_rng(seed)
    mask = np.zeros((2, n), dtype=np.uint8)
    last = (n - 1) // CHUNK * CHUNK            # first item of the last chunk
    for b in range(2):
        if kind == "ones":
            mask[b] = 1
        elif kind == "random35":
            mask[b] = rng.random(n) < 0.35
        elif kind == "one_in_last_chunk":
            mask[b, rng.integers(last, n)] = 1
        elif kind in ("chunk_of_64", "chunk_of_65"):
            # the survivors of ONE chunk number exactly 64 (a full group, no tail) or 65 (a group and a tail of one); the last
            # chunk that holds that many items, else the whole of a shorter input
            want = 64 if kind == "chunk_of_64" else 65
            first = last if n - last >= want else max(last - CHUNK, 0)
            size = min(CHUNK, n - first)
            mask[b, first + rng.choice(size, size=min(want, size), replace=False)] = 1
    return mask


@pytest.fixture(scope="module")
def dev(native_lib):
    from structure_from_motion_amd import device

    device.require_gpu()
    return device


@pytest.fixture(scope="module")
def stage(dev, native_lib):
    """Scenes, both pose tables, and per table and pair the decisions of ``sfm_cheirality`` and of the oracle on all N_MAX items
    (computed once; the tests slice them)."""
    sc = scenes()
    E = np.stack([s["E"].reshape(9) for s in sc])
    table, status = dev.decompose_essential(dev.to_device(E))
    assert status.cpu().tolist() == [0, 0]
    table = table.cpu().numpy()
    assert np.array_equal(table[:, 1::2, :9], table[:, 0::2, :9]) and np.array_equal(table[:, 1::2, 9:], -table[:, 0::2, 9:])
    tables = {"antipodal": table, "pose_by_pose": perturbed(table)}
    single, oracle = {}, {}
    for name, tab in tables.items():
        oracle[name] = np.stack([assert_margins(sc[b]["corr"], tab[b]) for b in range(2)])
        single[name] = np.stack([dev.cheirality(dev.to_device(sc[b]["corr"]), dev.to_device(tab[b]), THRESHOLD).cpu().numpy()
                                 for b in range(2)])
        assert np.array_equal(single[name].astype(bool), oracle[name]), name
    return dict(scenes=sc, tables=tables, single=single, oracle=oracle, lib=native_lib)


def cheirality_batched(dev, stage, table, n, mask):
    """``sfm_cheirality_batched`` on the first n items of both pairs -> [2, 4, n] uint8 (the output starts as 0xFF)."""
    from structure_from_motion_amd._native import check

    corr = dev.to_device(np.ascontiguousarray(np.stack([s["corr"][:n] for s in stage["scenes"]])))
    poses = dev.to_device(stage["tables"][table])
    mask_d = None if mask is None else dev.to_device(mask, torch.uint8)
    out = torch.full((2, 4, n), 0xFF, dtype=torch.uint8, device=corr.device)
    check(stage["lib"].sfm_cheirality_batched(corr.data_ptr(), n, 2, poses.data_ptr(), None if mask_d is None else mask_d.data_ptr(),
                                              THRESHOLD, out.data_ptr(), dev._stream()), "sfm_cheirality_batched")
    return out.cpu().numpy()


@pytest.mark.parametrize("n", N_VALUES)
def test_cheirality_batched_equals_single_call_and_oracle(dev, stage, n):
    for table in stage["tables"]:
        for kind in MASKS:
            mask = make_mask(kind, n, seed=n)
            got = cheirality_batched(dev, stage, table, n, mask)
            keep = np.ones((2, 1, n), dtype=bool) if mask is None else (mask != 0)[:, None, :]
            if kind == "one_in_last_chunk":
                assert keep.sum() == 2
            if kind in ("chunk_of_64", "chunk_of_65"):
                assert keep.sum() == 2 * min(n, int(kind[-2:]))
            assert np.all((got == 0) | (got == 1)), (table, kind)
            assert np.array_equal(got, np.where(keep, stage["single"][table][:, :, :n], 0)), (table, kind)
            assert np.array_equal(got.astype(bool), keep & stage["oracle"][table][:, :, :n]), (table, kind)


def vote_tables(dev, stage, n):
    """[4, 4, n]: the two pairs under a 35 % mask, a pair nobody passes, and a pair whose poses 1 and 3 tie ahead of 0 and 2."""
    real = cheirality_batched(dev, stage, "antipodal", n, make_mask("random35", n, seed=n))
    winner = real[0, int(np.argmax(real[0].sum(axis=1)))]
    tie = np.stack([np.zeros_like(winner), winner, np.zeros_like(winner), winner])
    return np.ascontiguousarray(np.stack([real[0], real[1], np.zeros_like(real[0]), tie]))


@pytest.mark.parametrize("skip", [None, "first", "last"])
@pytest.mark.parametrize("n", N_VALUES)
def test_pose_vote_counts_and_first_maximum(dev, stage, n, skip):
    from structure_from_motion_amd._native import check

    tables = vote_tables(dev, stage, n)
    B = tables.shape[0]
    index = None if skip is None else (0 if skip == "first" else n - 1)
    passes = dev.to_device(tables, torch.uint8)
    skip_d = None if index is None else dev.to_device(np.full(B, index, dtype=np.int32), torch.int32)
    votes = torch.full((B, 4), -7, dtype=torch.int32, device=passes.device)
    best = torch.full((B,), -7, dtype=torch.int32, device=passes.device)
    check(stage["lib"].sfm_pose_vote(passes.data_ptr(), n, B, None if skip_d is None else skip_d.data_ptr(), votes.data_ptr(),
                                     best.data_ptr(), dev._stream()), "sfm_pose_vote")
    counted = tables if index is None else np.delete(tables, index, axis=2)
    want = np.count_nonzero(counted, axis=2)
    want_best = np.where(want.max(axis=1) > 0, np.argmax(want, axis=1), -1)
    assert np.array_equal(votes.cpu().numpy(), want)
    assert np.array_equal(best.cpu().numpy(), want_best)
    assert want_best[2] == -1
    if want[3, 1] > 0:
        assert want[3, 1] == want[3, 3] and want_best[3] == 1   # the tie goes to the first maximum


@pytest.mark.parametrize("kind", ["random35", "ones"])
@pytest.mark.parametrize("n", N_VALUES)
def test_triangulate_selected_against_oracle(dev, stage, n, kind):
    from structure_from_motion_amd._native import check

    sc, table = stage["scenes"], stage["tables"]["antipodal"]
    two = cheirality_batched(dev, stage, "antipodal", n, make_mask(kind, n, seed=n + 1))
    pair = (0, 1, 0)                                       # the third pair is pair 0 again, without a pose
    passes = np.ascontiguousarray(two[list(pair)])
    best = np.array([int(np.argmax(stage["oracle"]["antipodal"][b].sum(axis=1))) for b in pair], dtype=np.int32)
    best[2] = -1
    pix_a = dev.to_device(np.ascontiguousarray(np.stack([sc[b]["pa"][:n] for b in pair])))
    pix_b = dev.to_device(np.ascontiguousarray(np.stack([sc[b]["pb"][:n] for b in pair])))
    K = np.ascontiguousarray(sc[0]["K"], dtype=np.float64)
    poses = dev.to_device(np.ascontiguousarray(table[list(pair)]))
    X = torch.full((3, n, 3), float("nan"), dtype=torch.float64, device=pix_a.device)
    valid = torch.full((3, n), 0xFF, dtype=torch.uint8, device=pix_a.device)
    best_d, passes_d = dev.to_device(best, torch.int32), dev.to_device(passes, torch.uint8)
    check(stage["lib"].sfm_triangulate_selected(pix_a.data_ptr(), pix_b.data_ptr(), n, 3, K.ctypes.data_as(C.c_void_p), poses.data_ptr(),
                                                best_d.data_ptr(), passes_d.data_ptr(), X.data_ptr(), valid.data_ptr(), dev._stream()),
          "sfm_triangulate_selected")
    X, valid = X.cpu().numpy(), valid.cpu().numpy()
    assert not X[2].any() and not valid[2].any()           # best = -1: all zeros (no NaN left either)
    for slot in (0, 1):
        b = pair[slot]
        chosen = passes[slot, best[slot]] != 0
        assert np.array_equal(valid[slot], chosen.astype(np.uint8))
        assert not X[slot][~chosen].any()
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = table[b, best[slot], :9].reshape(3, 3), table[b, best[slot], 9:]
        want = orc.triangulate_points(sc[b]["pa"][:n], sc[b]["pb"][:n], K, T)
        if chosen.any():   # the bar of test_triangulate_large_vs_oracle
            err = np.abs(X[slot][chosen] - want[chosen]) / np.linalg.norm(want[chosen], axis=1, keepdims=True)
            assert np.max(err) <= 1e-9
