"""The ragged similarity alignment on the GPU (csrc/sfm_align_models.hip): every pair against the single-pair
chain it is defined by (bit for bit), the filler and the statuses, refused offset tables, reproducibility and chunking, the NumPy
definition on the call's own tables, the public call and ``merge_frames`` on its result."""
import numpy as np
import pytest
import torch

import align_models_cases as cases
import similarity_cases as sc
import similarity_oracle as so

pytestmark = pytest.mark.gpu

SEED, STRIDE, H_BEGIN, RMS, ROUNDS = cases.SEED, cases.STRIDE, cases.H_BEGIN, cases.RMS, cases.ROUNDS
INT_SENTINEL, F64_SENTINEL, BYTE_SENTINEL = -99, 1e300, 77
Q = len(cases.SIZES)


@pytest.fixture(scope="module")
def dev(native_lib):
    from structure_from_motion_amd import device

    return device.require_gpu()


@pytest.fixture(scope="module")
def ragged(dev):
    """The fixture on the host and on the device (computed once, never written)."""
    from structure_from_motion_amd import device

    fx = cases.fixture()
    return dict(fx, pairs_t=device.to_device(fx["pairs"]), offset_t=device.to_device(fx["offset"], torch.int64),
                thr_t=device.to_device(fx["thr"]), min_extra_t=device.to_device(fx["min_extra"]))


def _prefilled(pairs, n_total, h, most, dev):
    from structure_from_motion_amd import device

    ws = device.AlignModelsWorkspace(pairs, n_total, h, most, dev)
    for t in ws.buffers():
        t.fill_(F64_SENTINEL if t.dtype == torch.float64 else (BYTE_SENTINEL if t.dtype == torch.uint8 else INT_SENTINEL))
    return ws


def _host(ws):
    return {name: t.cpu().numpy() for name, t in zip(cases.BUFFER_NAMES, ws.buffers())}


def _same(a, b):
    """Bit for bit, a NaN equal to any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float64:
        return a.shape == b.shape and bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def _assert_written(out):
    for name, a in out.items():
        sentinel = F64_SENTINEL if a.dtype == np.float64 else (BYTE_SENTINEL if a.dtype == np.uint8 else INT_SENTINEL)
        assert not np.any(a == sentinel), name


_CALLS = {}


def _call(ragged, dev, h, rounds=ROUNDS):
    """One ragged call on the fixture into poisoned buffers (once per (h, rounds), never written again): -> (out, records, infos)."""
    from structure_from_motion_amd import device

    if (h, rounds) not in _CALLS:
        ws = _prefilled(Q, len(ragged["pairs"]), h, max(cases.SIZES), dev)
        ws.run(ragged["pairs_t"], ragged["offset_t"], ragged["thr_t"], ragged["min_extra_t"], RMS, SEED, STRIDE, H_BEGIN, rounds)
        _CALLS[(h, rounds)] = (_host(ws), device.read_select(ws.result), device.read_similarity_refine_info(ws.info))
    return _CALLS[(h, rounds)]


def _assert_no_model(out, info, q, lo, hi):
    assert np.isnan(out["model_out"][q]).all() and out["model_out"][q].shape == (so.MODEL,), q
    assert not out["mask"][lo:hi].any() and not out["mask_out"][lo:hi].any(), q
    assert info[q].error == np.inf and (info[q].count, info[q].accepted, info[q].rounds_run) == (0, 0, 0), (q, info[q])
    assert out["info"][q].view(np.int32)[5] == 0   # reserved


def _assert_pass_filler(out, rec, q, h):
    f = cases.pass_filler(h)
    assert np.array_equal(out["S"][q], f["S"]) and np.isnan(out["model"][q]).all() and np.array_equal(out["flags"][q], f["flags"]), q
    assert np.array_equal(out["cnt"][q], f["cnt"]) and np.isnan(out["s1"][q]).all() and np.isnan(out["s2"][q]).all(), q
    assert rec[q].best_h == -1 and rec[q].best_err == np.inf and rec[q].best_cnt == 0, q
    assert rec[q].n_flagged == h and rec[q].first_flagged == 0 and rec[q].key == cases.NO_MODEL_KEY, q


def _chain(items, n, thr, gate, seed, h, rounds, dev):
    """The single-pair chain on one pair's items: the pass with a mask, then the refinement of its winner.  -> host arrays."""
    from structure_from_motion_amd import device

    ws = device.SimilarityWorkspace(1, n, h, dev)
    one = items.reshape(1, n, 6)
    ws.run(one, thr, gate, RMS, philox=(seed, H_BEGIN, STRIDE))
    ws.refine(one, thr, RMS, rounds)
    return {name: t[0].cpu().numpy() for name, t in zip(cases.BUFFER_NAMES[:-1], ws.buffers())}


PASS_NAMES = ("S", "model", "flags", "cnt", "s1", "s2", "result")


@pytest.mark.parametrize("rounds", [0, ROUNDS])
@pytest.mark.parametrize("h", cases.HS)
def test_equals_the_single_pair_chain(dev, ragged, h, rounds):
    """Every pair with at least three items bit for bit what SimilarityWorkspace.run and .refine give on it alone; for a pair
    without a winner everything up to the record, and the filler behind it."""
    out, rec, info = _call(ragged, dev, h, rounds)
    offset = ragged["offset"]
    for q, n in enumerate(cases.SIZES):
        lo, hi = offset[q], offset[q + 1]
        if n < so.SAMPLE:
            assert out["status"][q] == cases.TOO_FEW
            continue
        ref = _chain(ragged["pairs_t"][lo:hi], n, ragged["thr"][q], ragged["min_extra"][q], SEED + q * STRIDE, h, rounds, dev)
        for name in PASS_NAMES:
            assert _same(out[name][q], ref[name]), (q, name)
        assert np.array_equal(out["mask"][lo:hi], ref["mask"]), q
        assert out["status"][q] == cases.status_of(n, rec[q].best_h), q
        if rec[q].best_h < 0:
            assert not ref["mask"].any()
            _assert_no_model(out, info, q, lo, hi)
            continue
        assert _same(out["model_out"][q], ref["model_out"]), q
        assert np.array_equal(out["mask_out"][lo:hi], ref["mask_out"]), q
        assert np.array_equal(out["info"][q], ref["info"]), (q, out["info"][q], ref["info"])
        if rounds == 0:
            assert _same(out["model_out"][q], out["model"][q][rec[q].best_h]) and info[q].accepted == 0
            assert np.array_equal(out["mask_out"][lo:hi], (out["mask"][lo:hi] != 0).astype(np.uint8))
    assert out["status"][cases.NO_MODEL_PAIR] == cases.NO_MODEL
    # non-vacuity: every pair of 40 items or more but the gated one has a winner, and a refit round is kept somewhere
    assert all(out["status"][q] == cases.OK for q, n in enumerate(cases.SIZES) if n >= 40 and q != cases.NO_MODEL_PAIR)
    if rounds:
        assert any(info[q].accepted >= 1 for q in range(Q))
        assert info[cases.LARGEST].rounds_run >= 1


def test_tiny_pairs_with_winners(dev):
    """Pairs of 3, 4 and 5 clean items without a gate: each has a winner, and equals its chain."""
    from structure_from_motion_amd import device

    sizes, h = (3, 4, 5), 70
    scenes = [sc.scene(n, 70 + n, noise=1e-4) for n in sizes]
    pairs = np.concatenate([s[0] for s in scenes])
    offset = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    thr = np.array([sc.THR * s[1][0] ** 2 for s in scenes])
    gate = np.zeros(3)
    ws = _prefilled(3, len(pairs), h, 5, dev)
    pairs_t = device.to_device(pairs)
    ws.run(pairs_t, device.to_device(offset, torch.int64), device.to_device(thr), device.to_device(gate), RMS, SEED, STRIDE, H_BEGIN, ROUNDS)
    out = _host(ws)
    _assert_written(out)
    assert out["status"].tolist() == [cases.OK] * 3
    for q, n in enumerate(sizes):
        lo, hi = offset[q], offset[q + 1]
        ref = _chain(pairs_t[lo:hi], n, thr[q], 0.0, SEED + q * STRIDE, h, ROUNDS, dev)
        for name in PASS_NAMES + ("model_out", "info"):
            assert _same(out[name][q], ref[name]), (q, name)
        assert np.array_equal(out["mask"][lo:hi], ref["mask"]) and np.array_equal(out["mask_out"][lo:hi], ref["mask_out"]), q


def test_filler_and_every_element_written(dev, ragged):
    """No poison survives; the fillers of TOO_FEW, of NO_MODEL and of the items no pair owns are as defined."""
    h = cases.HS[0]
    out, rec, info = _call(ragged, dev, h)
    _assert_written(out)
    offset, N = ragged["offset"], len(ragged["pairs"])
    assert offset[0] == cases.FRONT > 0 and offset[-1] == N - cases.BACK < N
    for name in ("mask", "mask_out"):
        assert not out[name][:offset[0]].any() and not out[name][offset[-1]:].any(), name
    few = [q for q, n in enumerate(cases.SIZES) if n < so.SAMPLE]
    assert len(few) == 2
    for q in few:
        _assert_pass_filler(out, rec, q, h)
        _assert_no_model(out, info, q, offset[q], offset[q + 1])
        assert out["status"][q] == cases.TOO_FEW
    q = cases.NO_MODEL_PAIR
    assert out["status"][q] == cases.NO_MODEL and rec[q].best_h == -1 and rec[q].n_flagged < h
    assert np.isfinite(out["model"][q]).any() and (out["S"][q][:, :3] >= 0).all()   # its pass ran: only the winner is missing
    _assert_no_model(out, info, q, offset[q], offset[q + 1])
    assert set(np.unique(out["mask"])) <= {0, 1, 2} and set(np.unique(out["mask_out"])) <= {0, 1}


@pytest.mark.parametrize("table", ["decreasing", "past_the_end", "negative", "above_max_items"])
def test_bad_offset_tables(dev, ragged, table):
    """Ordinary inputs with a defined result: a status on every pair, the filler throughout, no error return, and nothing is
    read through the table."""
    from structure_from_motion_amd import device

    offset = ragged["offset"].copy()
    N, h, most = len(ragged["pairs"]), 70, max(cases.SIZES)
    if table == "decreasing":
        offset[6], offset[7] = offset[7], offset[6]
    elif table == "past_the_end":
        offset[-1] = N + 1
    elif table == "negative":
        offset[0] = -1
    else:
        most = max(cases.SIZES) - 1
    ws = _prefilled(Q, N, h, most, dev)
    ws.run(ragged["pairs_t"], device.to_device(offset, torch.int64), ragged["thr_t"], ragged["min_extra_t"], RMS, SEED, STRIDE, H_BEGIN,
           ROUNDS)
    out, rec, info = _host(ws), device.read_select(ws.result), device.read_similarity_refine_info(ws.info)
    _assert_written(out)
    assert np.all(device.read_align_status(ws.status) == device.ALIGN_BAD_OFFSETS)
    assert not out["mask"].any() and not out["mask_out"].any()
    for q in range(Q):
        _assert_pass_filler(out, rec, q, h)
        _assert_no_model(out, info, q, 0, N)


def test_reproducible_and_independent_of_chunking(dev, ragged):
    """Two calls give equal bytes, and the fixture split at every chunk boundary of chunk_bounds gives the bytes of the unsplit
    call."""
    from structure_from_motion_amd import device
    from structure_from_motion_amd.epipolar.view_graph import chunk_bounds

    h = cases.HS[0]
    out, _, _ = _call(ragged, dev, h)
    ws = _prefilled(Q, len(ragged["pairs"]), h, max(cases.SIZES), dev)
    ws.run(ragged["pairs_t"], ragged["offset_t"], ragged["thr_t"], ragged["min_extra_t"], RMS, SEED, STRIDE, H_BEGIN, ROUNDS)
    again = _host(ws)
    for name in cases.BUFFER_NAMES:
        assert out[name].tobytes() == again[name].tobytes(), name
    offset = ragged["offset"]
    for per_call in (1, 3, 4):
        chunks = chunk_bounds(Q, h, per_call * h)
        assert len(chunks) == -(-Q // per_call)
        for q0, q1 in chunks:
            lo, hi = int(offset[q0]), int(offset[q1])
            part = _prefilled(q1 - q0, hi - lo, h, max(cases.SIZES[q0:q1]), dev)
            part.run(ragged["pairs_t"][lo:hi], ragged["offset_t"][q0:q1 + 1] - lo, ragged["thr_t"][q0:q1], ragged["min_extra_t"][q0:q1],
                     RMS, SEED + q0 * STRIDE, STRIDE, H_BEGIN, ROUNDS)
            got = _host(part)
            for name in cases.BUFFER_NAMES:
                whole = out[name][lo:hi] if name in ("mask", "mask_out") else out[name][q0:q1]
                assert got[name].tobytes() == whole.tobytes(), (per_call, q0, name)


def test_against_the_numpy_definition(dev, ragged):
    """Per OK pair, on the call's own tables: cnt, s1 and s2 of the device's own models bit for bit; model_out within
    similarity_cases.PARITY_TOL (the tolerance DESIGN.md §6ag records) of the oracle's least-squares model of the same inlier set,
    reached by the oracle's refit rounds from the device's winner; no displaced item in mask_out and at least 99 % of the clean
    ones (tests/test_align_models_host.py shows that the oracle's own winner meets that share on this fixture)."""
    h = cases.HS[0]
    out, rec, info = _call(ragged, dev, h)
    offset = ragged["offset"]
    checked = 0
    for q, n in enumerate(cases.SIZES):
        if out["status"][q] != cases.OK:
            continue
        checked += 1
        lo, hi = offset[q], offset[q + 1]
        pairs, thr = ragged["pairs"][lo:hi], ragged["thr"][q]
        cnt, s1, s2 = so.score_table(pairs, out["model"][q], out["S"][q], thr)
        assert np.array_equal(out["cnt"][q], cnt), q
        assert _same(out["s1"][q], s1) and _same(out["s2"][q], s2), q
        best = rec[q].best_h
        assert best == so.select(cnt, s1, s2, out["flags"][q], ragged["min_extra"][q], RMS)[0], q
        assert np.array_equal(out["mask"][lo:hi], so.mask(pairs, out["model"][q], out["S"][q], best, thr)), q
        ref_model, ref_mask, ref = so.refine(pairs, out["model"][q][best], out["mask"][lo:hi], rec[q].best_err, thr, RMS, ROUNDS)
        gap = so.model_gap(out["model_out"][q], ref_model, pairs)
        print(f"pair {q} (n = {n}): gap to the oracle's refit {gap:.3e} (tolerance {sc.PARITY_TOL:.3e}), info {info[q]}, oracle {ref}")
        assert gap <= sc.PARITY_TOL, (q, gap)
        assert (info[q].accepted, info[q].rounds_run) == (ref["accepted"], ref["rounds_run"]), q
        kept, clean = out["mask_out"][lo:hi] != 0, ragged["clean"][q]
        assert info[q].count == np.count_nonzero(kept), q
        assert not kept[~clean].any(), q
        share = np.count_nonzero(kept[clean]) / np.count_nonzero(clean)
        assert share >= 0.99, (q, share)
    assert checked == sum(1 for n in cases.SIZES if n >= 40) - 1


def _sub_models(noise=5e-5):
    """Four sub-models of one cloud of 900 tracks, each in a frame and a unit of its own (model 0 in the world's), 20 % of each
    model's points displaced by at least 0.1 of its unit; five pairs, one of them reversed and one without a common id."""
    rng = np.random.default_rng(21)
    world = rng.uniform(-1.0, 1.0, size=(900, 3))
    ids = [np.arange(0, 400), np.arange(200, 600), np.concatenate([np.arange(400, 800), np.arange(0, 100)]), np.arange(600, 900)]
    truth = [(1.0, np.eye(3), np.zeros(3))] + [sc.similarity(30 + k) for k in (1, 2, 3)]   # world -> model k
    points, clean, order = [], [], []
    for k, mine in enumerate(ids):
        mine = rng.permutation(mine)                      # ids in no particular order
        s, R, t = truth[k]
        X = s * (world[mine] @ R.T) + t + rng.normal(scale=noise * s, size=(len(mine), 3))
        ok = np.ones(len(mine), dtype=bool)
        bad = rng.permutation(len(mine))[:len(mine) // 5]
        direction = rng.normal(size=(len(bad), 3))
        X[bad] += s * direction / np.linalg.norm(direction, axis=1, keepdims=True) * rng.uniform(0.1, 1.0, size=(len(bad), 1))
        ok[bad] = False
        points.append(X), clean.append(ok), order.append(mine)
    pairs = np.array([[0, 1], [1, 2], [2, 3], [2, 0], [1, 3]])
    thr = np.array([sc.THR * truth[j][0] ** 2 for _, j in pairs.tolist()])
    return world, truth, points, order, clean, pairs, thr


def test_public_call_and_merge(dev):
    """align_models equals estimate_similarity_with_ransac pair by pair, None where the status is not "ok"; merge_frames on its
    result puts every model's clean points within the threshold of the root's."""
    from structure_from_motion_amd.epipolar.view_graph import pair_min_extra
    from structure_from_motion_amd.multiview import alignment as al

    world, truth, points, ids, clean, pairs, thr = _sub_models()
    h, seed = 300, 11
    found = al.align_models(points, ids, pairs, thr, iterations=h, min_num_extra_inliers=5, min_extra_fraction=0.5, seed=seed,
                            max_hypotheses_per_call=2 * h)
    assert found.status == ["ok", "ok", "ok", "ok", "too_few"] and found.common_count.tolist() == [200, 200, 200, 100, 0]
    gate = pair_min_extra(found.common_count, 5, 0.5)
    for q, (i, j) in enumerate(pairs.tolist()):
        common, at_i, at_j = np.intersect1d(ids[i], ids[j], return_indices=True)
        assert np.array_equal(found.common_ids[q], common)
        got = found.estimate(q)
        if found.status[q] != "ok":
            assert got is None and np.isnan(found.scale[q]) and np.isnan(found.R[q]).all() and len(found.inliers[q]) == 0
            continue
        single = al.estimate_similarity_with_ransac(points[i][at_i], points[j][at_j], thr[q], iterations=h,
                                                    min_num_extra_inliers=int(gate[q]), seed=seed + q)
        assert single is not None
        assert got.scale == single.scale and np.array_equal(got.R, single.R) and np.array_equal(got.t, single.t), q
        assert np.array_equal(got.inliers, single.inliers) and got.error == single.error and got.refined == single.refined, q
        assert np.array_equal(found.inliers[q], common[single.inliers]) and found.inlier_count[q] == len(single.inliers)
        # no displaced point of either side among the inliers
        both = clean[i][at_i] & clean[j][at_j]
        assert both[single.inliers].all() and len(single.inliers) >= 0.99 * np.count_nonzero(both), q
    frames = al.merge_frames(4, pairs, found)
    assert frames.reached.all() and len(frames.tree_pairs) == 3 and 4 not in frames.tree_pairs.tolist()
    assert len(al.inconsistent_alignments(frames, 0.1, 1e-3)) == 0
    for k in range(4):
        merged = al.apply_similarity(frames.frame(k), points[k][clean[k]])
        worst = np.max(np.sum((merged - world[ids[k][clean[k]]]) ** 2, axis=1))
        print(f"model {k}: largest squared distance to the root's points {worst:.3e} (threshold {sc.THR:.1e})")
        assert worst <= sc.THR, (k, worst)
    # the same from one device call
    whole = al.align_models(points, ids, pairs, thr, iterations=h, min_num_extra_inliers=5, min_extra_fraction=0.5, seed=seed)
    for name in ("scale", "R", "t", "inlier_count", "error", "accepted", "ransac_count"):
        assert getattr(whole, name).tobytes() == getattr(found, name).tobytes(), name


def test_the_op(dev, ragged):
    """The functional op passes opcheck and agrees with the in-place one."""
    from structure_from_motion_amd import device, ops

    sizes = cases.SIZES[:cases.LARGEST]
    fx = cases.fixture(0, sizes)
    h, most = 33, max(sizes)
    args = (device.to_device(fx["pairs"]), device.to_device(fx["offset"], torch.int64), device.to_device(fx["thr"]),
            device.to_device(fx["min_extra"]))
    ws = _prefilled(len(sizes), len(fx["pairs"]), h, most, dev)
    ws.run(*args, RMS, SEED, STRIDE, H_BEGIN, ROUNDS)
    op = ops.load()
    tail = (most, device._as_int64(SEED), STRIDE, H_BEGIN)
    model_out, mask_out, info, status, mask, result = op.align_models(*args, *tail, h, RMS, ROUNDS)
    for got, name in ((model_out, "model_out"), (mask_out, "mask_out"), (info, "info"), (status, "status"), (mask, "mask"),
                      (result, "result")):
        assert got.cpu().numpy().tobytes() == getattr(ws, name).cpu().numpy().tobytes(), name
    tests = ("test_schema", "test_faketensor")
    torch.library.opcheck(op.align_models.default, args + tail + (9, RMS, ROUNDS), test_utils=tests)
    small = device.AlignModelsWorkspace(len(sizes), len(fx["pairs"]), 9, most, dev)
    torch.library.opcheck(op.align_models_.default, args + tail + (RMS, ROUNDS) + small.buffers(), test_utils=tests)
