"""The ragged two-view pass over a match graph on the GPU (csrc/sfm_view_graph.hip): every pair against the two
single-pair passes it is defined by, the selection, mask and verdict definitions on the call's own tables, the small pairs'
filler, the model kinds and the seed pair, chunking, refused offset tables, the other passes, the op and the app."""
import numpy as np
import pytest
import torch

import homography_oracle as ho
import view_graph_oracle as vo
from structure_from_motion_amd import synthetic

pytestmark = pytest.mark.gpu

K = synthetic.BENCH_K
THR = vo.THR
SEED, STRIDE, H_BEGIN = 0x9E3779B97F4A7C15, 3, 5
MAX_RATIO = 0.8
INT_SENTINEL, F64_SENTINEL, BYTE_SENTINEL = -99, 1e300, 77


@pytest.fixture(scope="module")
def dev(native_lib):
    from structure_from_motion_amd import device

    return device.require_gpu()


def _ragged(scenes, sizes):
    from structure_from_motion_amd import device

    corr, offset, min_extra = vo.ragged_arrays(scenes)
    return dict(scenes=scenes, sizes=sizes, corr=corr, offset=offset, min_extra=min_extra, corr_t=device.to_device(corr),
                offset_t=device.to_device(offset, torch.int64), min_extra_t=device.to_device(min_extra))


@pytest.fixture(scope="module")
def ragged(dev):
    """The 12-pair fixture on the host and on the device (computed once, never written)."""
    return _ragged(vo.ragged_scenes(), vo.SIZES)


@pytest.fixture(scope="module")
def ragged_special(dev):
    """12 pairs on the special motions and planes of tests/homography_cases.py."""
    return _ragged(vo.ragged_scenes(vo.SPECIAL_SIZES, scenes=vo.SPECIAL_SCENES), vo.SPECIAL_SIZES)


def _prefilled(pairs, n_total, h, dev):
    from structure_from_motion_amd import device

    ws = device.ViewGraphWorkspace(pairs, n_total, h, dev)
    for t in ws.buffers():
        t.fill_(F64_SENTINEL if t.dtype == torch.float64 else (BYTE_SENTINEL if t.dtype == torch.uint8 else INT_SENTINEL))
    return ws


def _host(ws):
    names = ("S", "H", "E", "h_flags", "h_cnt", "h_s1", "h_s2", "e_flags", "e_cnt", "e_s1", "e_s2", "h_result", "e_result",
             "h_mask", "e_mask", "verdict")
    return {name: t.cpu().numpy() for name, t in zip(names, ws.buffers())}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _assert_written(out):
    for name, a in out.items():
        sentinel = F64_SENTINEL if a.dtype == np.float64 else (BYTE_SENTINEL if a.dtype == np.uint8 else INT_SENTINEL)
        assert not np.any(a == sentinel), name


# h: both sides of the scoring kernel's 256-lane block
@pytest.mark.parametrize("h, fixture", [pytest.param(h, f, id=f"{h}{tag}")
                                        for f, tag in (("ragged", ""), ("ragged_special", "-special")) for h in (1, 255, 257)])
def test_equals_the_single_pair_passes(dev, request, fixture, h):
    from structure_from_motion_amd import device

    ragged = request.getfixturevalue(fixture)
    corr, offset, min_extra, sizes = ragged["corr"], ragged["offset"], ragged["min_extra"], ragged["sizes"]
    Q, N = len(sizes), len(corr)
    ws = _prefilled(Q, N, h, dev)
    ws.run(ragged["corr_t"], ragged["offset_t"], ragged["min_extra_t"], THR, vo.RMS, MAX_RATIO, SEED, STRIDE, H_BEGIN)
    out = _host(ws)
    _assert_written(out)
    h_rec, e_rec, verdicts = device.read_select(ws.h_result), device.read_select(ws.e_result), ws.read_verdicts()
    for q, n in enumerate(sizes):
        lo, hi = offset[q], offset[q + 1]
        c = corr[lo:hi]
        S = out["S"][q]
        if n >= 4:   # the homography pass of this pair alone
            c_t = ragged["corr_t"][lo:hi].reshape(1, n, 4)
            hws = device.HomographyWorkspace(1, n, h, dev)
            hws.run(c_t, THR, min_extra[q], vo.RMS, philox=(SEED + q * STRIDE, H_BEGIN, STRIDE))
            assert np.array_equal(S, hws.S[0].cpu().numpy()), q
            assert np.array_equal(_bits(out["H"][q]), _bits(hws.H[0].cpu().numpy())), q
            assert np.array_equal(out["h_flags"][q], hws.flags[0].cpu().numpy()), q
            assert np.array_equal(out["h_cnt"][q], hws.cnt[0].cpu().numpy()), q
            # the same loop over the same items in the same order
            assert np.array_equal(_bits(out["h_s1"][q]), _bits(hws.s1[0].cpu().numpy())), q
            assert np.array_equal(_bits(out["h_s2"][q]), _bits(hws.s2[0].cpu().numpy())), q
        else:
            assert np.all(S == -1) and np.all(out["h_flags"][q] == 1) and np.isnan(out["H"][q]).all()
            assert np.all(out["h_cnt"][q] == 0) and np.isnan(out["h_s1"][q]).all() and np.isnan(out["h_s2"][q]).all()
        if n >= 6:   # the five-point pass on the rows the homography pass stored
            ews = device.RansacWorkspace(1, n, h, dev)
            ews.S.copy_(hws.S)
            ews.run(c_t, THR, min_extra[q], vo.RMS, solver="five_point")
            assert np.array_equal(_bits(out["E"][q]), _bits(ews.E[0].cpu().numpy())), q
            assert np.array_equal(out["e_flags"][q], ews.flags[0].cpu().numpy()), q
            assert np.array_equal(out["e_cnt"][q], ews.cnt[0].cpu().numpy()), q
            # the existing SED kernel sums in another order: the suite's tolerance between SED kernels
            np.testing.assert_allclose(out["e_s1"][q], ews.s1[0].cpu().numpy(), rtol=1e-12, atol=0.0, equal_nan=True)
            np.testing.assert_allclose(out["e_s2"][q], ews.s2[0].cpu().numpy(), rtol=1e-12, atol=0.0, equal_nan=True)
        else:
            assert np.all(out["e_flags"][q] == 1) and np.isnan(out["E"][q]).all()
            assert np.all(out["e_cnt"][q] == 0) and np.isnan(out["e_s1"][q]).all() and np.isnan(out["e_s2"][q]).all()
        # winners: the select definition on the call's own tables
        for rec, name, sample in ((h_rec[q], "h", vo.H_SAMPLE), (e_rec[q], "e", vo.E_SAMPLE)):
            cnt = out[name + "_cnt"][q]
            best, err = vo.select(cnt, out[name + "_s1"][q], out[name + "_s2"][q], out[name + "_flags"][q], min_extra[q], sample)
            assert rec.best_h == best, (q, name)
            if best >= 0:
                assert abs(rec.best_err - err) <= 1e-15 * err and rec.best_cnt == cnt[best], (q, name)
            else:
                assert rec.best_err == np.inf and rec.best_cnt == 0
            if n < sample:
                assert best == -1 and rec.n_flagged == h and rec.first_flagged == 0
        # masks: the mask definitions for those winners
        assert np.array_equal(out["h_mask"][lo:hi], ho.mask(c, out["H"][q], S, h_rec[q].best_h, THR)), q
        assert np.array_equal(out["e_mask"][lo:hi], vo.essential_mask(c, out["E"][q], S, e_rec[q].best_h, THR)), q
        # the verdict follows from the two records
        kind, hc, ec, ratio = vo.verdict(h_rec[q].best_h, h_rec[q].best_cnt, e_rec[q].best_h, e_rec[q].best_cnt, MAX_RATIO)
        v = verdicts[q]
        assert (v.kind, v.homography_count, v.essential_count, v.ratio, v.reserved) == (kind, hc, ec, ratio, 0), q
        if n < 4:
            assert v.kind == vo.NONE and h_rec[q].best_h == -1 and e_rec[q].best_h == -1
    if h >= 255:   # the fixture is not vacuous: the large pairs have both models
        assert all(h_rec[q].best_h >= 0 and e_rec[q].best_h >= 0 for q in range(Q) if sizes[q] >= 300)


def test_model_kinds_and_seed_pair(dev):
    from structure_from_motion_amd.epipolar import view_graph as vg

    cases = (("pan10", 400), ("plane_bench", 350), ("bench", 250), ("bench", 120), ("gen12", 90))
    scenes = [ho.motion_scene(name, n, 7, 0.5, 0.3) for name, n in cases]
    features, pairs, matches = vo.match_graph(scenes)
    graph = vg.verify_pairs(K, features, pairs, matches, THR, min_num_extra_inliers=[max(8, n // 15) for _, n in cases],
                            max_iterations=200, seed=5)
    print("kinds", graph.kind, "H", graph.homography_count, "E", graph.essential_count, "ratio", graph.ratio)
    assert graph.kind == ["homography", "homography", "essential", "essential", "homography"]
    # the margins of the single-pair model-choice test
    assert all(graph.ratio[q] >= 0.9 for q in (0, 1, 4)) and all(graph.ratio[q] <= 0.5 for q in (2, 3))
    assert int(np.argmax(graph.essential_count)) == 0   # the pan has the most essential inliers and no baseline
    assert vg.choose_seed_pair(graph) == 2
    for q in range(5):
        chosen = graph.essential_inliers[q] if graph.kind[q] == "essential" else graph.homography_inliers[q]
        assert np.array_equal(graph.inlier_matches[q], chosen)
        assert len(graph.essential_inliers[q]) == graph.essential_count[q]
        assert len(graph.homography_inliers[q]) == graph.homography_count[q]
        assert np.isfinite(graph.E[q]).all() and np.isfinite(graph.H[q]).all()


def _same(a, b):
    assert a.kind == b.kind and np.array_equal(a.pairs, b.pairs)
    for name in ("E", "H", "ratio"):
        assert np.array_equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name
    assert np.array_equal(a.essential_count, b.essential_count) and np.array_equal(a.homography_count, b.homography_count)
    for name in ("essential_inliers", "homography_inliers", "inlier_matches"):
        assert all(np.array_equal(x, y) for x, y in zip(getattr(a, name), getattr(b, name))), name


def test_chunking_and_determinism(dev, ragged):
    from structure_from_motion_amd.epipolar import view_graph as vg

    features, pairs, matches = vo.match_graph(ragged["scenes"])
    h = 64
    assert len(vg.chunk_bounds(len(pairs), h, 4 * h)) == 3
    args = (K, features, pairs, matches, THR)
    whole = vg.verify_pairs(*args, min_extra_fraction=1.0 / 15.0, max_iterations=h, seed=11)
    _same(whole, vg.verify_pairs(*args, min_extra_fraction=1.0 / 15.0, max_iterations=h, seed=11))
    _same(whole, vg.verify_pairs(*args, min_extra_fraction=1.0 / 15.0, max_iterations=h, seed=11, max_hypotheses_per_call=4 * h))
    assert whole.kind[:2] == ["none", "none"] and "none" not in whole.kind[7:]
    assert all(len(m) == 0 for m in whole.inlier_matches[:2])


@pytest.mark.parametrize("table", ["decreasing", "past_the_end", "negative"])
def test_bad_offsets_are_a_status(dev, ragged, table):
    from structure_from_motion_amd import device

    offset = ragged["offset"].copy()
    Q, N, h = len(vo.SIZES), len(ragged["corr"]), 65
    if table == "decreasing":
        offset[8], offset[9] = offset[9], offset[8]
    elif table == "past_the_end":
        offset[-1] = N + 1
    else:
        offset[0] = -1
    ws = _prefilled(Q, N, h, dev)
    ws.run(ragged["corr_t"], device.to_device(offset, torch.int64), ragged["min_extra_t"], THR, vo.RMS, MAX_RATIO, SEED)
    out = _host(ws)
    _assert_written(out)
    for v in ws.read_verdicts():
        assert (v.kind, v.homography_count, v.essential_count, v.ratio) == (vo.BAD_OFFSETS, 0, 0, np.inf)
    assert all(r.best_h == -1 for r in device.read_select(ws.h_result) + device.read_select(ws.e_result))
    assert not out["h_mask"].any() and not out["e_mask"].any()
    assert np.all(out["S"] == -1) and np.isnan(out["H"]).all() and np.isnan(out["E"]).all()
    outcome = ws.outcome()
    assert np.all(outcome.kind == device.PAIR_BAD_OFFSETS) and np.isnan(outcome.H).all() and np.isnan(outcome.E).all()


def test_items_no_pair_owns(dev):
    """5 items in front of offset[0] and 7 behind offset[pairs], around pairs of 4, 0, 7 and 513 items (one item past a 512-item
    score tile) with 70 hypotheses (one fit block of 64 and a partial one): both mask bytes of an item no pair owns are 0, and
    every other byte of every buffer is that of the call on the same pairs without those items."""
    from structure_from_motion_amd import device

    sizes, h, front, back = (4, 0, 7, 513), 70, 5, 7
    corr, offset, min_extra = vo.ragged_arrays(vo.ragged_scenes(sizes))

    def call(c, o):
        ws = _prefilled(len(sizes), len(c), h, dev)
        ws.run(device.to_device(c), device.to_device(o, torch.int64), device.to_device(min_extra), THR, vo.RMS, MAX_RATIO, SEED, STRIDE,
               H_BEGIN)
        out = _host(ws)
        _assert_written(out)
        return out
    plain = call(corr, offset)
    # the unowned items are copies of the large pair's: owned by mistake, they would be marked like them
    padded = call(np.concatenate([corr[-front:], corr, corr[-back:]]), offset + front)
    assert plain["h_mask"][-513:].any() or plain["e_mask"][-513:].any()   # not vacuous: the large pair has a winner
    for name in plain:
        if name in ("h_mask", "e_mask"):
            assert not padded[name][:front].any() and not padded[name][-back:].any(), name
            assert np.array_equal(padded[name][front:-back], plain[name]), name
        else:
            assert padded[name].tobytes() == plain[name].tobytes(), name


def test_other_passes_are_untouched_and_opcheck(dev, ragged):
    """One essential, one five-point and one homography single-pair pass before and after a ragged call on the same stream leave
    bit-equal records; the op passes opcheck."""
    import random

    from structure_from_motion_amd import device, ops

    n, h = 600, 256
    sc = ho.motion_scene("bench", n, 31, 0.5, 0.3)
    c = device.to_device(sc["corr"][None])
    table = device.to_device(device.PyShuffleTable(n, h, random.Random(8), advance=False).S[None], torch.int32)

    def others():
        kept = []
        for solver in ("eight_point", "five_point", "homography"):
            ws = device.HomographyWorkspace(1, n, h, dev) if solver == "homography" else device.RansacWorkspace(1, n, h, dev)
            ws.S.copy_(table)
            if solver == "homography":
                ws.run(c, THR, 10, vo.RMS)
            else:
                ws.run(c, 1.5e-6, 10, vo.RMS, solver=solver)
            kept += [t.clone() for t in (ws.result, ws.cnt, ws.s1.view(torch.int64), ws.s2.view(torch.int64),
                                         ws.model.view(torch.int64), ws.flags, ws.mask)]
        return kept

    before = others()
    Q, N = len(vo.SIZES), len(ragged["corr"])
    ws = device.ViewGraphWorkspace(Q, N, 128, dev)
    ws.run(ragged["corr_t"], ragged["offset_t"], ragged["min_extra_t"], THR, vo.RMS, MAX_RATIO, SEED)
    assert ws.outcome().kind[-1] != device.PAIR_NONE
    after = others()
    assert all(before[k][0, 1] >= 0 for k in (0, 7))   # both essential passes found a model (a homography need not, on this scene)
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    small = device.ViewGraphWorkspace(Q, N, 9, dev)
    args = (ragged["corr_t"], ragged["offset_t"], ragged["min_extra_t"], 5, 1, 0, THR, vo.RMS, MAX_RATIO) + small.buffers()
    torch.library.opcheck(ops.load().verify_pairs_.default, args, test_utils=("test_schema", "test_faketensor"))


def test_app_batched_route(dev):
    from apps import sfm_multi_view as app

    loop = app.run(tracks="matches")
    batched = app.run(tracks="matches", verify="batched")
    assert "pairs_none" not in loop["track_build"]
    build = batched["track_build"]
    print("loop", loop["rotation_error_rad"], loop["translation_error"], "batched", batched["rotation_error_rad"],
          batched["translation_error"], build)
    assert batched["views_registered"] == 8
    assert max(batched["rotation_error_rad"].values()) <= max(loop["rotation_error_rad"].values()) + 2e-3
    assert max(batched["translation_error"].values()) <= max(loop["translation_error"].values()) + 2e-2
    assert build["pure_track_fraction"] >= 0.9
    assert build["pairs_none"] == 0 and build["pairs_essential"] + build["pairs_homography"] == build["pairs_kept"] == 18
