"""What the host and GPU tests of the ragged similarity alignment share (tests/test_align_models_host.py,
tests/test_gpu_align_models.py; csrc/sfm_align_models.hip): the ragged fixture, the oracle's filler rules, hand-made
alignments for ``merge_frames`` and the stream case of ``sfm_align_models``."""
import functools

import numpy as np

import similarity_cases as sc
import similarity_oracle as so
import stream_cases

SEED, STRIDE, H_BEGIN = sc.SEED, sc.STRIDE, sc.H_BEGIN
RMS, ROUNDS = sc.RMS, 2
HS = (100, 257)   # neither a multiple of the 64-lane fit block or the 256-lane score block
# 2 048 / 2 049: the step from one reduction block to two; 4 100: three blocks; 262 145: the first size beyond the 128-block cap
SIZES = (40, 0, 2, 3, 4, 513, 2048, 2049, 4100, 262145)
NO_MODEL_PAIR = SIZES.index(513)   # its gate is its item count: nobody passes
LARGEST = SIZES.index(262145)
FRONT, BACK = 5, 7                 # items before offset[0] and behind offset[Q] that no pair owns
OK, NO_MODEL, TOO_FEW, BAD_OFFSETS = range(4)
STATUS = ("ok", "no_model", "too_few", "bad_offsets")
BUFFER_NAMES = ("S", "model", "flags", "cnt", "s1", "s2", "result", "mask", "model_out", "mask_out", "info", "status")
NO_MODEL_KEY = 0x7FFFFFFFFFFFFFFF   # sfm_select_result.key without a winner


@functools.lru_cache(maxsize=None)
def fixture(seed=0, sizes=SIZES):
    """The ragged fixture (computed once, never written): every pair with at least one item is a scene of its own —
    similarity_cases.scene(n, seed, outliers=0.3, noise=1e-4), a similarity per pair — under its own threshold, similarity_cases.THR
    times the square of its scale.  -> dict(pairs (N, 6) with FRONT + BACK unowned items, offset (Q + 1,), thr (Q,), min_extra (Q,),
    sims, clean (per pair bool masks))."""
    rng = np.random.default_rng(1000 + seed)
    blocks, sims, clean, thr, gate = [rng.uniform(-1.0, 1.0, size=(FRONT, 6))], [], [], [], []
    for q, n in enumerate(sizes):
        pairs, sim, ok = sc.scene(n, seed + 17 * q + 1, outliers=0.3, noise=1e-4) if n else (np.zeros((0, 6)), sc.similarity(1000 + q), np.zeros(0, bool))
        blocks.append(pairs)
        sims.append(sim)
        clean.append(ok)
        thr.append(sc.THR * sim[0] * sim[0])
        # 513: nobody passes.  3 and 4: one extra inlier, which a pair with a displaced item among so few cannot have — without a
        # gate its winner is a sample that holds the displaced item (tests/test_gpu_align_models.py has tiny pairs with winners)
        gate.append(float(n) if n == 513 else (1.0 if n <= 4 else 10.0))
    blocks.append(rng.uniform(-1.0, 1.0, size=(BACK, 6)))
    offset = FRONT + np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    out = dict(pairs=np.ascontiguousarray(np.concatenate(blocks)), offset=offset, thr=np.array(thr), min_extra=np.array(gate),
               sims=sims, clean=clean, sizes=tuple(sizes))
    return out


def status_of(n, best_h):
    return TOO_FEW if n < so.SAMPLE else (OK if best_h >= 0 else NO_MODEL)


def pass_filler(h):
    """The tables of a pair too small for a sample."""
    return dict(S=np.full((h, 8), -1, dtype=np.int32), model=np.full((h, so.MODEL), np.nan),
                flags=np.full(h, so.FIT_DEGENERATE, dtype=np.int32), cnt=np.zeros(h, dtype=np.int32), s1=np.full(h, np.nan),
                s2=np.full(h, np.nan))


def alignments(sims, counts, centroids=None, status=None):
    """A hand-made ``ModelAlignments`` for ``merge_frames``: one (s, R, t) and one inlier count per pair."""
    from structure_from_motion_amd.multiview.alignment import ModelAlignments

    Q = len(sims)
    counts = np.asarray(counts, dtype=np.int64)
    return ModelAlignments(
        scale=np.array([s for s, _, _ in sims], dtype=np.float64), R=np.array([R for _, R, _ in sims], dtype=np.float64).reshape(Q, 3, 3),
        t=np.array([t for _, _, t in sims], dtype=np.float64).reshape(Q, 3), status=list(status or ["ok"] * Q), inlier_count=counts,
        inliers=[np.arange(c) for c in counts], common_count=counts.copy(), ransac_count=counts.copy(), error=np.zeros(Q),
        accepted=np.zeros(Q, dtype=np.int64), common_ids=[np.arange(c) for c in counts],
        centroid=np.zeros((Q, 3)) if centroids is None else np.asarray(centroids, dtype=np.float64))


# The op list is empty on purpose, as for register_views (tests/register_views_cases.py): tests/test_stream_cases_host.py requires
# every op a case names to be in ops.FUNCTIONAL_OPS / INPLACE_OPS, two tuples that an earlier schema guard pins, and the ops of
# this call are listed in ops.ALIGN_MODELS_OPS.  The calls below still go through them, and their outputs are compared.
@stream_cases.case(["sfm_align_models"], [])
def align_models(dev):
    """The fixture without its largest pair, two scenes of equal shapes and two seeds: the C entry point on the test's buffers
    and workspace, and the functional op on the same inputs (outputs only)."""
    import torch

    from structure_from_motion_amd import device, ops

    i = stream_cases.Inst(dev)
    # three spare streams of torch's pool beside this case: four in all, so that every later side stream of
    # tests/test_gpu_streams.py keeps its hardware queue (the comment in tests/register_views_cases.py)
    i.keep_alignment = [torch.cuda.Stream() for _ in range(3)]
    sizes = SIZES[:LARGEST] + SIZES[LARGEST + 1:]
    a, b = fixture(0, sizes), fixture(100, sizes)
    assert np.array_equal(a["offset"], b["offset"]) and np.array_equal(a["min_extra"], b["min_extra"])
    Q, N, h, most = len(sizes), len(a["pairs"]), 257, max(sizes)
    pairs, thr = i.inp(a["pairs"], b["pairs"]), i.inp(a["thr"], b["thr"])
    offset, min_extra = i.same(a["offset"], torch.int64), i.same(a["min_extra"])
    shapes = device.AlignModelsWorkspace(Q, N, h, most, dev)
    out = [i.out(name, tuple(buf.shape), buf.dtype) for name, buf in zip(BUFFER_NAMES, shapes.buffers())]
    lib = stream_cases._lib()
    ws = i.work(lib.sfm_align_models_workspace_bytes(N, Q, most))
    i.host = {"A": SEED, "B": SEED + 1}
    # the fillers of the pairs below the sample size and no degenerate sample elsewhere; the sizes and the gates fix every status
    i.constant |= {"flags", "status"}
    op = ops.load()

    def call():
        stream_cases._check(lib.sfm_align_models(i.cur, STRIDE, H_BEGIN, pairs.data_ptr(), N, offset.data_ptr(), Q, most, thr.data_ptr(),
                                                 min_extra.data_ptr(), h, RMS, ROUNDS, *[t.data_ptr() for t in out], ws.data_ptr(),
                                                 ws.numel(), stream_cases._st()), "sfm_align_models")
        returned = op.align_models(pairs, offset, thr, min_extra, most, device._as_int64(i.cur), STRIDE, H_BEGIN, h, RMS, ROUNDS)
        return stream_cases.Returned(returned[:3] + returned[4:])   # (the statuses are the same in both scenes)
    i.call = call
    return i
