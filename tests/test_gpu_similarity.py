"""The similarity alignment on the GPU (csrc/sfm_similarity.hip) against the NumPy definition of
tests/similarity_oracle.py: the fit per hypothesis, scoring bit for bit, selection and mask, the Philox route, special motions,
outliers, the masked fit, the refinement, the refusals and the public call."""
import numpy as np
import pytest
import torch

import similarity_cases as cases   # registers the stream cases of the three entry points (tests/test_gpu_streams.py runs them)
import similarity_oracle as so

pytestmark = pytest.mark.gpu

THR, RMS = cases.THR, cases.RMS
POISON = 0xAB
SFM_EINVAL = -1   # include/sfm_hip.h
# A model gap g (so.model_gap) moves every residual by at most g times the natural length of side B, which is below 10 for the
# fixtures of this module (|t| <= 3 sqrt(3), s |a| <= 2 sqrt(3)): the bound on the difference of two RMS errors.
LENGTH = 10.0


@pytest.fixture(scope="module")
def dev(native_lib):
    from structure_from_motion_amd import device

    return device.require_gpu()


def _poisoned(ws):
    for buf in ws.buffers():
        buf.view(torch.uint8).fill_(POISON)
    return ws


def _workspace(dev, pairs, h):
    from structure_from_motion_amd import device

    B, n = pairs.shape[:2]
    return _poisoned(device.SimilarityWorkspace(B, n, h, dev))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else a.dtype)


def _same_doubles(a, b):
    """Bit for bit, a NaN equal to any NaN (its sign and payload are not part of the definition)."""
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(_bits(a)[~nan], _bits(b)[~nan])


def _host(ws):
    return {k: t.cpu().numpy() for k, t in zip(("S", "model", "flags", "cnt", "s1", "s2", "result", "mask"), ws.buffers())}


def _compare_models(got, ref, flags, ratios, pairs, what):
    """Flags equal; unflagged models within PARITY_TOL, leaving out at most NEAR_CAP of them as near-degenerate."""
    near = cases.near_degenerate(ratios)
    assert np.mean(near) <= cases.NEAR_CAP, what
    worst = 0.0
    for k in np.nonzero((flags == 0) & ~near)[0]:
        worst = max(worst, so.model_gap(got[k], ref[k], pairs))
    print(what, "largest gap to the oracle", worst, "tolerance", cases.PARITY_TOL)
    assert worst <= cases.PARITY_TOL, what
    return worst


def _check_pass_against_oracle(dev, pairs, out, thr, gate, seeds, h_begin, what):
    """Everything a pass wrote for pairs (B, n, 6) against the oracle, the device's own models on both sides of the scoring."""
    from structure_from_motion_amd import device

    B, n = pairs.shape[:2]
    h = out["S"].shape[1]
    records = device.read_select(torch.as_tensor(out["result"]))
    for b in range(B):
        S = so.sample_table(seeds[b], h_begin, h, n) if seeds is not None else out["S"][b]
        assert np.array_equal(out["S"][b], S), (what, b)
        models, flags, ratios = so.fit(pairs[b], S)
        assert np.array_equal(out["flags"][b], flags), (what, b)
        _compare_models(out["model"][b], models, flags, ratios, pairs[b], (what, b))
        assert not np.any(_bits(out["model"][b]) == _bits(np.frombuffer(bytes([POISON]) * 8, dtype=np.float64))[0])
        cnt, s1, s2 = so.score_table(pairs[b], out["model"][b], S, thr)
        assert np.array_equal(out["cnt"][b], cnt), (what, b)
        assert _same_doubles(out["s1"][b], s1) and _same_doubles(out["s2"][b], s2), (what, b)
        best, err = so.select(cnt, s1, s2, flags, gate, RMS)
        rec = records[b]
        assert rec.best_h == best and rec.n_flagged == int(np.count_nonzero(flags)), (what, b)
        if best >= 0:
            assert rec.best_err == err and rec.best_cnt == cnt[best]
        assert np.array_equal(out["mask"][b], so.mask(pairs[b], out["model"][b], S, best, thr)), (what, b)


@pytest.mark.parametrize("shape", cases.PARITY_SHAPES, ids=str)
def test_pass_parity(dev, shape):
    """Philox samples, fit, scoring, selection and mask of a whole pass; entry b samples from seed + b * stride."""
    from structure_from_motion_amd import device

    B, n, h = shape
    pairs = cases.parity_fixture(shape)
    gate = min(10, n - 3)
    ws = _workspace(dev, pairs, h)
    items = device.to_device(pairs)
    ws.run(items, THR, gate, RMS, philox=(cases.SEED, cases.H_BEGIN, cases.STRIDE))
    out = _host(ws)
    seeds = [cases.SEED + b * cases.STRIDE for b in range(B)]
    _check_pass_against_oracle(dev, pairs, out, THR, gate, seeds, cases.H_BEGIN, shape)
    # every aggregation: the record equals the oracle's selection over the device's own tables
    for method in range(4):
        records = device.read_select(device.select_best(ws.cnt, ws.s1, ws.s2, ws.flags, gate, method, sample_size=3))
        for b in range(B):
            best, err = so.select(out["cnt"][b], out["s1"][b], out["s2"][b], out["flags"][b], gate, method)
            assert records[b].best_h == best and (best < 0 or records[b].best_err == err), (shape, method, b)
    # the same pass fed the table it wrote; entry b alone with its own seed
    fed = _workspace(dev, pairs, h)
    fed.S.copy_(ws.S)
    fed.run(items, THR, gate, RMS)
    for name, a, b_ in zip("S model flags cnt s1 s2 result mask".split(), ws.buffers(), fed.buffers()):
        assert torch.equal(a.view(torch.uint8), b_.view(torch.uint8)), (shape, name)
    for b in range(B):
        one = _workspace(dev, pairs[b:b + 1], h)
        one.run(items[b:b + 1].contiguous(), THR, gate, RMS, philox=(seeds[b], cases.H_BEGIN, cases.STRIDE))
        for name, a, b_ in zip("S model flags cnt s1 s2 result mask".split(), ws.buffers(), one.buffers()):
            assert torch.equal(a[b].view(torch.uint8), b_[0].view(torch.uint8)), (shape, name, b)


@pytest.mark.parametrize("kind", ["nan_item", "nan_threshold", "no_mask"])
def test_pass_with_nan_rows(dev, kind):
    """A NaN item gives NaN models (flagged) in the samples that hold it and a NaN error under every other model; a NaN
    threshold passes nothing.  Scoring stays the oracle's bit for bit."""
    from structure_from_motion_amd import device

    shape = (1, 64, 257)
    pairs = cases.parity_fixture(shape).copy()
    thr = THR
    if kind == "nan_item":
        pairs[0, 5, 4] = np.nan
    if kind == "nan_threshold":
        thr = float("nan")
    ws = _workspace(dev, pairs, 257)
    ws.run(device.to_device(pairs), thr, 0, RMS, with_mask=kind != "no_mask", philox=(7, 0, 1))
    out = _host(ws)
    if kind == "no_mask":
        assert np.all(out["mask"] == POISON)   # a null mask is not written
        out["mask"] = so.mask(pairs[0], out["model"][0], out["S"][0], int(out["result"][0, 1]), thr)[None]
    _check_pass_against_oracle(dev, pairs, out, thr, 0, [7], 0, kind)
    if kind == "nan_item":
        assert np.count_nonzero(out["flags"]) >= 1 and np.isnan(out["s1"][0][out["flags"][0] != 0]).all()
    if kind == "nan_threshold":
        assert not out["cnt"].any()


@pytest.mark.parametrize("name", list(cases.special_motions()))
def test_special_motions(dev, name):
    """Each motion fits: every hypothesis agrees with the oracle, the winner holds every pair, and the least-squares model of
    all pairs is the oracle's."""
    from structure_from_motion_amd import device

    pairs, sim = cases.special_motions()[name]
    n, h = len(pairs), 64
    # the threshold in the squared units of side B: the clouds of scale 1e3 and 1e-3 and the one 1e6 units out are exact to
    # about eps times their coordinates, far below it
    thr = THR * max(sim[0], 1.0) ** 2 if name != "scale_1e-3" else THR * 1e-6
    ws = _workspace(dev, pairs[None], h)
    items = device.to_device(pairs[None])
    ws.run(items, thr, n // 2, RMS, philox=(cases.SEED, 0, 1))
    out = _host(ws)
    _check_pass_against_oracle(dev, pairs[None], out, thr, n // 2, [cases.SEED], 0, name)
    assert int(out["result"][0, 1]) >= 0 and np.all(out["mask"] != 0) and not out["flags"].any()
    model, flags = device.fit_similarity(items)
    ref, flag, _ = so.model_svd(pairs[:, :3], pairs[:, 3:])
    assert int(flags.cpu()[0]) == flag == 0
    gap = so.model_gap(model[0].cpu().numpy(), ref, pairs)
    print(name, "least-squares gap to the oracle", gap)
    assert gap <= cases.PARITY_TOL


def test_a_mirror_image_has_no_winner(dev):
    from structure_from_motion_amd import device

    pairs = cases.mirror_pairs()
    ws = _workspace(dev, pairs[None], 64)
    ws.run(device.to_device(pairs[None]), THR, len(pairs) // 2, RMS, philox=(5, 0, 1))
    out = _host(ws)
    _check_pass_against_oracle(dev, pairs[None], out, THR, len(pairs) // 2, [5], 0, "mirror")
    assert int(out["result"][0, 1]) == -1 and not out["mask"].any() and not out["flags"].any()
    dets = [np.linalg.det(m[:9].reshape(3, 3)) for m in out["model"][0]]
    assert np.max(np.abs(np.array(dets) - 1.0)) < 1e-12   # proper rotations only
    assert ws.outcome().best_h == -1


def test_outliers_noise_free(dev):
    """30 % of side B displaced by at least 100 x the threshold: the winner's inliers are exactly the clean set and the model
    is the truth; the refined model is the least-squares model of the clean set."""
    from structure_from_motion_amd import device

    pairs, sim, clean, h, gate, seed = cases.outlier_fixture()
    truth = np.concatenate([sim[1].reshape(9), sim[2], [sim[0]]])
    ws = _workspace(dev, pairs[None], h)
    items = device.to_device(pairs[None])
    ws.run(items, THR, gate, RMS, philox=(seed, 0, 1))
    model_out, mask_out, info = ws.refine(items, THR, RMS, rounds=2)
    outcome = ws.outcome()
    assert outcome.best_h >= 0 and np.array_equal(outcome.mask != 0, clean)
    assert so.model_gap(outcome.model, truth, pairs) <= cases.PARITY_TOL
    assert np.array_equal(mask_out[0].cpu().numpy() != 0, clean)
    fitted, flags = device.fit_similarity(items, device.to_device(clean.astype(np.uint8), torch.uint8).reshape(1, -1))
    assert int(flags.cpu()[0]) == 0
    refined = model_out[0].cpu().numpy()
    assert so.model_gap(refined, fitted[0].cpu().numpy(), pairs) <= cases.PARITY_TOL
    assert so.model_gap(refined, truth, pairs) <= cases.PARITY_TOL
    rec = device.read_similarity_refine_info(info)[0]
    assert rec.count == int(np.count_nonzero(clean)) and rec.rounds_run >= 1


# ---------------------------------------------------------------------------------------------------------------------
# the masked fit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 513, 5000])
def test_masked_fit(dev, n):
    """Parity with the oracle; a null mask is an all-ones mask bit for bit; repeated calls give the same bytes (5000 items
    take three blocks of partial sums per entry)."""
    from structure_from_motion_amd import device

    B = 3
    pairs, _, clean = cases.batch_scene(B, n, 170 + n, outliers=0.3, noise=3e-4)
    items = device.to_device(pairs)
    mask = device.to_device(clean.astype(np.uint8), torch.uint8)
    model, flags = device.fit_similarity(items, mask)
    again = device.fit_similarity(items, mask)
    assert torch.equal(model.view(torch.int64), again[0].view(torch.int64)) and torch.equal(flags, again[1])
    everything, _ = device.fit_similarity(items, None)
    ones, _ = device.fit_similarity(items, torch.ones_like(mask))
    assert torch.equal(everything.view(torch.int64), ones.view(torch.int64))
    got, worst = model.cpu().numpy(), 0.0
    for b in range(B):
        ref, flag, _ = so.model_svd(pairs[b, clean[b], :3], pairs[b, clean[b], 3:])
        assert int(flags[b]) == flag == 0
        worst = max(worst, so.model_gap(got[b], ref, pairs[b]))
        all_ref, _, _ = so.model_svd(pairs[b, :, :3], pairs[b, :, 3:])
        worst = max(worst, so.model_gap(everything[b].cpu().numpy(), all_ref, pairs[b]))
    print(n, "largest gap to the oracle", worst)
    assert worst <= cases.PARITY_TOL


def test_masked_fit_flags_sets_that_determine_nothing(dev):
    from structure_from_motion_amd import device

    pairs, _, _ = cases.scene(64, 3)
    pairs = np.stack([pairs] * 4)
    pairs[1, :, :3] = np.outer(np.linspace(-1.0, 1.0, 64), np.array([1.0, -2.0, 0.5])) + 0.3   # side A collinear
    pairs[2, :, 3:] = 1.0                                                                        # side B coincident
    mask = np.ones((4, 64), dtype=np.uint8)
    mask[0, 2:] = 0      # two items
    mask[3] = 0          # none
    model = torch.full((4, 13), 7.0, dtype=torch.float64, device=dev)
    flags = torch.full((4,), 7, dtype=torch.int32, device=dev)
    device.fit_similarity(device.to_device(pairs), device.to_device(mask, torch.uint8), out=(model, flags))
    assert flags.cpu().tolist() == [1, 1, 1, 1]
    assert not np.any(model.cpu().numpy() == 7.0)   # every model is written as it comes out


# ---------------------------------------------------------------------------------------------------------------------
# the refinement
# ---------------------------------------------------------------------------------------------------------------------
def _refine_inputs(dev, B, n, h=64):
    from structure_from_motion_amd import device

    pairs = cases.batch_scene(B, n, 90 + n, outliers=0.3, noise=3e-4)[0]
    items = device.to_device(pairs)
    ws = device.SimilarityWorkspace(B, n, h, dev)
    ws.run(items, THR, 10, RMS, philox=(11, 0, 1))
    rows = torch.arange(B, device=dev)
    best = ws.result[:, 1]
    assert int(best.min()) >= 0
    return pairs, items, ws.model[rows, best].contiguous(), ws.mask.clone(), ws.result[:, 2].contiguous().view(torch.float64).clone()


@pytest.mark.parametrize("n", [513, 5000])
def test_refine_parity_and_reproducibility(dev, n):
    from structure_from_motion_amd import device

    B = 3
    pairs, items, model, mask, err = _refine_inputs(dev, B, n)
    out = device.similarity_refine(items, model, mask, err, THR, RMS, rounds=3)
    again = device.similarity_refine(items, model, mask, err, THR, RMS, rounds=3)
    for a, b in zip(out, again):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    infos = device.read_similarity_refine_info(out[2])
    kept = 0
    for b in range(B):
        ref_model, ref_mask, ref = so.refine(pairs[b], model[b].cpu().numpy(), mask[b].cpu().numpy(), float(err[b]), THR, RMS, 3)
        got = infos[b]
        print(n, b, got, ref)
        assert (got.count, got.accepted, got.rounds_run) == (ref["count"], ref["accepted"], ref["rounds_run"])
        assert abs(got.error - ref["error"]) <= cases.PARITY_TOL * LENGTH
        assert so.model_gap(out[0][b].cpu().numpy(), ref_model, pairs[b]) <= cases.PARITY_TOL
        assert np.array_equal(out[1][b].cpu().numpy(), ref_mask)
        kept += got.accepted
    assert kept >= 1   # the accept rule keeps a round on these scenes
    # rounds = 0 copies
    model_out, mask_out, info = device.similarity_refine(items, model, mask, err, THR, RMS, rounds=0)
    assert torch.equal(model_out.view(torch.int64), model.view(torch.int64)) and torch.equal(mask_out, (mask != 0).to(torch.uint8))
    for b, rec in enumerate(device.read_similarity_refine_info(info)):
        assert (rec.error, rec.count, rec.accepted, rec.rounds_run) == (float(err[b]), int(torch.count_nonzero(mask[b])), 0, 0)
    assert int(info.view(torch.int32)[:, 5].abs().max()) == 0   # reserved


def test_refine_rejects_a_round_and_stops_early(dev):
    """Entry 0: the input is already the least-squares model of its inliers and claims an error of 0, so the round is
    rejected and model_out is model_in bit for bit.  Entry 1: two inliers.  Entry 2: a collinear inlier set.  Entry 3: none."""
    from structure_from_motion_amd import device

    n = 64
    pairs, _, _ = cases.scene(n, 21, noise=3e-4)
    pairs = np.stack([pairs] * 4)
    pairs[2, :10, :3] = np.outer(np.linspace(-1.0, 1.0, 10), np.array([1.0, -2.0, 0.5])) + 0.3
    mask = np.zeros((4, n), dtype=np.uint8)
    mask[0] = 1
    mask[1, :2] = 2
    mask[2, :10] = 1
    items = device.to_device(pairs)
    fitted, _ = device.fit_similarity(items[:1].contiguous())
    model = torch.cat([fitted, fitted, fitted, fitted]).contiguous()
    err = torch.tensor([0.0, 1.0, 1.0, 1.0], dtype=torch.float64, device=dev)
    model_out = torch.full((4, 13), 7.0, dtype=torch.float64, device=dev)
    mask_out = torch.full((4, n), POISON, dtype=torch.uint8, device=dev)
    info = torch.full((4, 3), -1, dtype=torch.int64, device=dev)
    device.similarity_refine(items, model, device.to_device(mask, torch.uint8), err, 1.0, RMS, rounds=3, out=(model_out, mask_out, info))
    assert torch.equal(model_out.view(torch.int64), model.view(torch.int64))
    assert np.array_equal(mask_out.cpu().numpy(), (mask != 0).astype(np.uint8))
    recs = device.read_similarity_refine_info(info)
    assert [(r.error, r.count, r.accepted, r.rounds_run) for r in recs] == [(0.0, n, 0, 1), (1.0, 2, 0, 0), (1.0, 10, 0, 1), (1.0, 0, 0, 0)]


# ---------------------------------------------------------------------------------------------------------------------
# refusals, the public call
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing_and_leave_the_outputs_untouched(dev, native_lib):
    from structure_from_motion_amd import device

    lib = native_lib
    B, n, h = 1, 64, 8
    pairs = device.to_device(cases.scene(n, 2)[0][None])
    ws = _workspace(dev, pairs, h)
    work = torch.full((1 << 16,), POISON, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    p = [t.data_ptr() for t in ws.buffers()]
    S, model, flags, cnt, s1, s2, result, mask, model_out, mask_out, info = p

    def run_pass(n=n, h=h, batch=B, agg=RMS, pairs_p=pairs.data_ptr(), model_p=model):
        return lib.sfm_similarity_ransac_pass(1, 1, 1, 0, pairs_p, n, h, batch, THR, 0.0, agg, S, model_p, flags, cnt, s1, s2, result, mask, st)

    def run_fit(n=n, batch=B, pairs_p=pairs.data_ptr(), ws_bytes=work.numel()):
        return lib.sfm_similarity_fit_masked(pairs_p, n, batch, None, model_out, flags, work.data_ptr(), ws_bytes, st)

    def run_refine(n=n, batch=B, agg=RMS, rounds=2, ws_bytes=work.numel(), info_p=info):
        return lib.sfm_similarity_refine(pairs.data_ptr(), n, batch, model, mask, s1, THR, agg, rounds, model_out, mask_out, info_p,
                                         work.data_ptr(), ws_bytes, st)
    refused = [run_pass(n=2), run_pass(n=-1), run_pass(h=-1), run_pass(batch=-1), run_pass(agg=9), run_pass(pairs_p=None),
               run_pass(model_p=None), run_fit(n=2), run_fit(batch=-1), run_fit(pairs_p=None), run_fit(ws_bytes=16),
               run_refine(n=2), run_refine(agg=-1), run_refine(rounds=-1), run_refine(ws_bytes=16), run_refine(info_p=None)]
    assert refused == [SFM_EINVAL] * len(refused)
    torch.cuda.synchronize()
    for buf in ws.buffers() + (work,):
        assert bool((buf.view(torch.uint8) == POISON).all())


# Round-off of carrying the scene below into another frame and projecting again, measured with the NumPy helpers on the true
# similarity: the squared pixel errors (at most 4.3 px^2, pixels of order 1e3) move by at most 5.8e-13 px^2; held to ten times.
END_TO_END_ROUNDOFF = 5.8e-13


def test_public_call_end_to_end(dev):
    """Frame B is frame A under a known similarity with a quarter of its points wrong: the estimate is the truth, and B's
    poses and points carried back by it reproject exactly as they did."""
    from lib.multiview import alignment
    from structure_from_motion_amd import synthetic

    sc = synthetic.multi_view_scene(views=5, points=120, seed=4, outlier_fraction=0.0)
    K = np.asarray(synthetic.BENCH_K, dtype=np.float64)
    poses_a, points_a = np.asarray(sc["poses_true"]), np.asarray(sc["points_true"])
    cam, pt, pixels = sc["camera_indices"], sc["point_indices"], sc["pixels"]
    truth = cases.similarity(33)
    points_b = alignment.apply_similarity(truth, points_a)
    poses_b = alignment.transform_poses(truth, poses_a)
    extent = float(np.max(np.abs(points_b - points_b.mean(axis=0))))
    wrong = points_b.copy()
    bad = np.random.default_rng(1).permutation(len(wrong))[:30]
    wrong[bad] += extent * np.random.default_rng(2).uniform(0.2, 1.0, size=(30, 3))
    thr = (1e-6 * extent) ** 2
    est = alignment.estimate_similarity_with_ransac(points_a, wrong, thr, iterations=256, seed=3)
    assert est is not None and est.refined in (True, False)
    assert np.array_equal(est.inliers, np.setdiff1d(np.arange(len(wrong)), bad))
    row = np.concatenate([est.R.reshape(9), est.t, [est.scale]])
    assert so.model_gap(row, np.concatenate([truth[1].reshape(9), truth[2], [truth[0]]]), np.hstack([points_a, points_b])) <= cases.PARITY_TOL
    before = cases.reprojection_errors(poses_b, points_b, cam, pt, pixels, K)
    back = alignment.invert(est)
    after = cases.reprojection_errors(alignment.transform_poses(back, poses_b), alignment.apply_similarity(back, points_b), cam, pt, pixels, K)
    moved = float(np.max(np.abs(after - before)))
    print("reprojection errors moved by", moved, "largest", float(np.max(before)))
    assert moved <= 10.0 * END_TO_END_ROUNDOFF
    # no model: a gate nobody passes, and fit_similarity on the corrupted pairs is visibly worse than the robust estimate
    assert alignment.estimate_similarity_with_ransac(points_a, wrong, thr, iterations=64, min_num_extra_inliers=len(wrong), seed=3) is None
    plain = alignment.fit_similarity(points_a, wrong)
    assert plain.error > 1e3 * np.sqrt(thr)
    with pytest.raises(alignment.SimilarityCalculationError):
        alignment.fit_similarity(np.outer(np.arange(5.0), np.ones(3)), points_b[:5])
