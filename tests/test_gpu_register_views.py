"""The ragged absolute-pose call on the GPU (csrc/sfm_register_views.hip): every view against the single-view
chain it is defined by (bit for bit), the selection, mask and refinement definitions on the call's own tables, the filler and
statuses, refine_rounds = 0, chunking, refused offset tables, the other passes, the op and the app."""
import numpy as np
import pytest
import torch

import pnp_oracle as po
import register_views_cases as cases
import register_views_oracle as rv

pytestmark = pytest.mark.gpu

K, THR, RMS = rv.K, rv.THR, rv.RMS
SEED, STRIDE, H_BEGIN = cases.SEED, cases.STRIDE, cases.H_BEGIN
ROUNDS, MAX_STEPS = cases.ROUNDS, cases.MAX_STEPS
INT_SENTINEL, F64_SENTINEL, BYTE_SENTINEL = -99, 1e300, 77
HS = (1, 255, 257)   # both sides of the scoring kernel's 256-lane block


@pytest.fixture(scope="module")
def dev(native_lib):
    from structure_from_motion_amd import device

    return device.require_gpu()


@pytest.fixture(scope="module")
def ragged(dev):
    """The 12-view fixture on the host and on the device (computed once, never written)."""
    from structure_from_motion_amd import device

    fx = rv.fixture(0)
    pts, offset, min_extra = rv.ragged_arrays(fx)
    return dict(fx=fx, pts=pts, offset=offset, min_extra=min_extra, pts_t=device.to_device(pts),
                offset_t=device.to_device(offset, torch.int64), min_extra_t=device.to_device(min_extra))


def _prefilled(views, n_total, h, dev):
    from structure_from_motion_amd import device

    ws = device.RegisterViewsWorkspace(views, n_total, h, dev)
    for t in ws.buffers():
        t.fill_(F64_SENTINEL if t.dtype == torch.float64 else (BYTE_SENTINEL if t.dtype == torch.uint8 else INT_SENTINEL))
    return ws


def _host(ws):
    return {name: t.cpu().numpy() for name, t in zip(cases.BUFFER_NAMES, ws.buffers())}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _assert_written(out):
    for name, a in out.items():
        sentinel = F64_SENTINEL if a.dtype == np.float64 else (BYTE_SENTINEL if a.dtype == np.uint8 else INT_SENTINEL)
        assert not np.any(a == sentinel), name


_CALLS = {}


def _call(ragged, dev, h, rounds=ROUNDS):
    """One ragged call on the fixture into sentinel-filled buffers (once per (h, rounds), never written again): -> (out, records,
    infos)."""
    from structure_from_motion_amd import device

    if (h, rounds) not in _CALLS:
        ws = _prefilled(len(rv.SIZES), len(ragged["pts"]), h, dev)
        ws.run(ragged["pts_t"], ragged["offset_t"], ragged["min_extra_t"], K, THR, RMS, SEED, STRIDE, H_BEGIN, rounds, MAX_STEPS)
        _CALLS[(h, rounds)] = (_host(ws), device.read_select(ws.result), device.read_pnp_refine_info(ws.info))
    return _CALLS[(h, rounds)]


def _info_row(out, v):
    """(error bits, count, accepted, lm_steps, reserved) of view v from the int64 [V, 3] view of the records."""
    raw = out["info"][v].tobytes()
    return (np.frombuffer(raw, dtype=np.int64, count=1)[0],) + tuple(np.frombuffer(raw, dtype=np.int32, offset=8, count=4).tolist())


def _assert_no_model(out, info, v, lo, hi):
    assert np.isnan(out["pose_out"][v]).all(), v
    assert not out["mask"][lo:hi].any() and not out["mask_out"][lo:hi].any(), v
    assert info[v].error == np.inf and (info[v].count, info[v].accepted, info[v].lm_steps) == (0, 0, 0), (v, info[v])
    assert _info_row(out, v)[4] == 0


def _assert_pass_filler(out, rec, v, h):
    f = rv.pass_filler(h)
    assert np.array_equal(out["S"][v], f["S"]) and np.isnan(out["model"][v]).all() and np.array_equal(out["flags"][v], f["flags"]), v
    assert np.array_equal(out["cnt"][v], f["cnt"]) and np.isnan(out["s1"][v]).all() and np.isnan(out["s2"][v]).all(), v
    assert rec[v].best_h == -1 and rec[v].best_err == np.inf and rec[v].best_cnt == 0, v
    assert rec[v].n_flagged == h and rec[v].first_flagged == 0 and rec[v].key == rv.NO_MODEL_KEY, v


@pytest.mark.parametrize("h", HS)
def test_equals_the_single_view_chain(dev, ragged, h):
    """Every element written; every view bit for bit what PnPWorkspace.run(solver="p3p") and .refine give on it alone."""
    from structure_from_motion_amd import device

    out, rec, info = _call(ragged, dev, h)
    _assert_written(out)
    offset, min_extra = ragged["offset"], ragged["min_extra"]
    for v, n in enumerate(rv.SIZES):
        lo, hi = offset[v], offset[v + 1]
        if n < rv.SAMPLE:
            _assert_pass_filler(out, rec, v, h)
            _assert_no_model(out, info, v, lo, hi)
            assert out["status"][v] == rv.TOO_FEW
            continue
        p_t = ragged["pts_t"][lo:hi].reshape(1, n, 5)
        ws = device.PnPWorkspace(1, n, h, dev)
        ws.run(p_t, K, THR, min_extra[v], RMS, philox=(SEED + v * STRIDE, H_BEGIN, STRIDE), solver="p3p")
        assert np.array_equal(out["S"][v], ws.S[0].cpu().numpy()), v
        assert np.array_equal(_bits(out["model"][v]), _bits(ws.model[0].cpu().numpy())), v
        assert np.array_equal(out["flags"][v], ws.flags[0].cpu().numpy()), v
        assert np.array_equal(out["cnt"][v], ws.cnt[0].cpu().numpy()), v
        assert np.array_equal(_bits(out["s1"][v]), _bits(ws.s1[0].cpu().numpy())), v
        assert np.array_equal(_bits(out["s2"][v]), _bits(ws.s2[0].cpu().numpy())), v
        assert np.array_equal(out["result"][v], ws.result[0].cpu().numpy()), v
        assert np.array_equal(out["mask"][lo:hi], ws.mask[0].cpu().numpy()), v
        assert out["status"][v] == rv.status_of(n, rec[v].best_h), v
        if rec[v].best_h < 0:
            _assert_no_model(out, info, v, lo, hi)
            continue
        model, mask, single = ws.refine(p_t, K, THR, RMS, rounds=ROUNDS, max_steps=MAX_STEPS)
        assert np.array_equal(_bits(out["pose_out"][v]), _bits(model[0].cpu().numpy())), v
        assert np.array_equal(out["mask_out"][lo:hi], mask[0].cpu().numpy()), v
        assert np.array_equal(out["info"][v], single[0].cpu().numpy()), v
    assert out["status"][rv.OUTLIER_VIEW] == rv.NO_MODEL
    if h >= 255:   # non-vacuity: the large views all have a winner, and a refinement round is kept somewhere
        assert all(rec[v].best_h >= 0 for v, n in enumerate(rv.SIZES) if n >= 300)
        assert any(info[v].accepted >= 1 for v, n in enumerate(rv.SIZES) if n >= 300)
        assert out["status"][rv.PLANAR_VIEW] == rv.OK


@pytest.mark.parametrize("h", HS)
def test_definitions_on_the_calls_own_tables(dev, ragged, h):
    """The record against the select definition, the mask against the mask definition, pose_out and mask_out against
    pnp_refine_oracle from the winner's row and the seed mask, at the tolerance tests/test_gpu_pnp_refine.py holds that oracle
    to: 1e-9 on R, 1e-9 max(1, |t|) on t, the masks equal off the items within 1e-9 THR of the threshold."""
    out, rec, info = _call(ragged, dev, h)
    offset, min_extra, pts = ragged["offset"], ragged["min_extra"], ragged["pts"]
    for v, n in enumerate(rv.SIZES):
        lo, hi = offset[v], offset[v + 1]
        p, S, model = pts[lo:hi], out["S"][v], out["model"][v]
        cnt = out["cnt"][v]
        best, err = rv.select(cnt, out["s1"][v], out["s2"][v], out["flags"][v], min_extra[v])
        assert rec[v].best_h == best, v
        if best < 0:
            assert rec[v].best_err == np.inf and rec[v].best_cnt == 0, v
            continue
        assert abs(rec[v].best_err - err) <= 1e-15 * err and rec[v].best_cnt == cnt[best], v
        assert np.array_equal(out["mask"][lo:hi], rv.pnp_mask(p, model, S, best)), v
        seed = rv.seed_mask(out["mask"][lo:hi], S, best)
        ref = rv.refine(p, model[best], seed, rec[v].best_err, ROUNDS, MAX_STEPS)
        R, t = out["pose_out"][v][:9].reshape(3, 3), out["pose_out"][v][9:]
        assert np.max(np.abs(R - ref["R"])) <= 1e-9, (v, np.max(np.abs(R - ref["R"])))
        assert np.max(np.abs(t - ref["t"])) <= 1e-9 * max(1.0, np.max(np.abs(ref["t"]))), v
        assert info[v].accepted == ref["accepted"], (v, info[v], ref["accepted"])
        e = po.score_values(ref["R"], ref["t"], K, p)
        with np.errstate(invalid="ignore"):
            borderline = np.abs(e - THR) <= 1e-9 * THR
        assert np.array_equal(out["mask_out"][lo:hi][~borderline], ref["mask"][~borderline]), v
        assert abs(info[v].count - ref["count"]) <= int(np.count_nonzero(borderline)), v
        if not borderline.any():
            assert info[v].count == ref["count"] == int(out["mask_out"][lo:hi].sum()), v
            assert abs(info[v].error - ref["error"]) <= 1e-9 * abs(ref["error"]), v
        if n < rv.MIN_ITEMS + 1:   # at most five seed items once item 3 has left: never refined
            assert (info[v].accepted, info[v].lm_steps) == (0, 0), v


def test_no_refinement_rounds(dev, ragged):
    """refine_rounds = 0: pose_out is the winner's bytes, mask_out the mask rule, nothing accepted and no step taken."""
    h = 255
    out, rec, info = _call(ragged, dev, h, rounds=0)
    _assert_written(out)
    full, _, _ = _call(ragged, dev, h)
    for name in ("S", "model", "flags", "cnt", "s1", "s2", "result", "mask", "status"):   # the pass does not depend on the rounds
        assert out[name].tobytes() == full[name].tobytes(), name
    offset = ragged["offset"]
    winners = 0
    for v, n in enumerate(rv.SIZES):
        lo, hi = offset[v], offset[v + 1]
        best = rec[v].best_h
        if best < 0:
            _assert_no_model(out, info, v, lo, hi)
            continue
        winners += 1
        assert np.array_equal(_bits(out["pose_out"][v]), _bits(out["model"][v][best])), v
        seed = rv.seed_mask(out["mask"][lo:hi], out["S"][v], best)
        assert np.array_equal(out["mask_out"][lo:hi], seed), v
        assert (info[v].count, info[v].accepted, info[v].lm_steps) == (int(seed.sum()), 0, 0), v
        assert _bits(info[v].error) == _bits(rec[v].best_err), v
    assert winners >= 8


def test_chunking_and_determinism(dev, ragged):
    """register_views on the shuffled fixture: one, five and all views per device call, and a repeated call, give equal bytes;
    the inliers come back as ascending indices into the caller's arrays."""
    from structure_from_motion_amd.pnp.registration import register_views

    points, view, index, pixels = rv.observations(ragged["fx"], shuffle_seed=5)
    h, V = 64, len(rv.SIZES)

    def run(per_call):
        return register_views(K, points, view, index, pixels, THR, num_views=V, min_num_extra_inliers=2, min_extra_fraction=1 / 15,
                              max_iterations=h, seed=SEED, max_hypotheses_per_call=per_call * h)
    results = [run(1), run(5), run(V), run(V)]
    first = results[0]
    for other in results[1:]:
        for a, b in zip(first, other):
            if isinstance(a, list) and a and isinstance(a[0], np.ndarray):
                assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
            elif isinstance(a, list):
                assert a == b
            else:
                assert a.tobytes() == b.tobytes()
    assert first.status[:2] == ["too_few", "too_few"] and first.status[rv.OUTLIER_VIEW] == "no_model"
    assert all(first.status[v] == "ok" for v, n in enumerate(rv.SIZES) if n >= 300)
    for v, n in enumerate(rv.SIZES):
        mine = first.inliers[v]
        assert np.all(view[mine] == v) and np.all(np.diff(mine) > 0) and len(mine) == first.inlier_count[v], v
        if first.status[v] != "ok":
            assert np.isnan(first.poses[v]).all() and len(mine) == 0 and first.ransac_count[v] == 0 and first.error[v] == np.inf
            continue
        assert first.ransac_count[v] >= rv.SAMPLE and np.isfinite(first.poses[v]).all()
        # the inliers are the observations within the threshold under the returned pose
        p = np.column_stack([points[index[mine]], pixels[mine]])
        assert np.all(po.score_values(first.poses[v][:9].reshape(3, 3), first.poses[v][9:], K, p) <= THR * (1 + 1e-9)), v
        # and the pose is the view's own: 0.5 px of noise at f = 1520 px is 3e-4 rad per observation, far less over 200 inliers,
        # while another solution of the sample is off by hundredths of a radian
        if n >= 300:
            truth = ragged["fx"]["views"][v]
            assert np.max(np.abs(first.poses[v][:9].reshape(3, 3) - truth["R"])) < 5e-3, v


@pytest.mark.parametrize("table", ["decreasing", "past_the_end", "negative"])
def test_bad_offset_tables(dev, ragged, table):
    """A status on every view, the filler throughout, and nothing is read through the table."""
    from structure_from_motion_amd import device

    offset = ragged["offset"].copy()
    N, V, h = len(ragged["pts"]), len(rv.SIZES), 70
    if table == "decreasing":
        offset[7], offset[8] = offset[8], offset[7]
    elif table == "past_the_end":
        offset[-1] = N + 1
    else:
        offset[0] = -1
    ws = _prefilled(V, N, h, dev)
    ws.run(ragged["pts_t"], device.to_device(offset, torch.int64), ragged["min_extra_t"], K, THR, RMS, SEED, STRIDE, H_BEGIN, ROUNDS,
           MAX_STEPS)
    out, rec, info = _host(ws), device.read_select(ws.result), device.read_pnp_refine_info(ws.info)
    _assert_written(out)
    assert np.all(device.read_register_status(ws.status) == device.REGISTER_BAD_OFFSETS)
    assert not out["mask"].any() and not out["mask_out"].any()
    for v in range(V):
        _assert_pass_filler(out, rec, v, h)
        _assert_no_model(out, info, v, 0, N)


def test_items_no_view_owns(dev):
    """5 items in front of offset[0] and 7 behind offset[views], around views of 4, 0, 7 and 513 items (one item past a 512-item
    score tile) with 70 hypotheses (one fit block of 64 and a partial one): both mask bytes of an item no view owns are 0, and
    every other byte of every buffer is that of the call on the same views without those items."""
    from structure_from_motion_amd import device

    sizes, h, front, back = (4, 0, 7, 513), 70, 5, 7
    pts, offset, min_extra = rv.ragged_arrays(rv.fixture(3, sizes))

    def call(p, o):
        ws = _prefilled(len(sizes), len(p), h, dev)
        ws.run(device.to_device(p), device.to_device(o, torch.int64), device.to_device(min_extra), K, THR, RMS, SEED, STRIDE, H_BEGIN,
               ROUNDS, MAX_STEPS)
        out = _host(ws)
        _assert_written(out)
        return out
    plain = call(pts, offset)
    # the unowned items are copies of the large view's: owned by mistake, they would be marked like them
    padded = call(np.concatenate([pts[-front:], pts, pts[-back:]]), offset + front)
    assert plain["status"].tolist()[1::2] == [rv.TOO_FEW, rv.OK] and plain["mask_out"][-513:].any()   # not vacuous
    for name in plain:
        if name in ("mask", "mask_out"):
            assert not padded[name][:front].any() and not padded[name][-back:].any(), name
            assert np.array_equal(padded[name][front:-back], plain[name]), name
        else:
            assert padded[name].tobytes() == plain[name].tobytes(), name


def test_other_passes_are_untouched_and_the_op(dev, ragged):
    """The single-view P3P pass and pnp_refine give their earlier bytes after a ragged call on the same stream; the functional op
    passes opcheck and agrees with the in-place one."""
    from structure_from_motion_amd import device, ops

    n, h = 700, 130
    view = device.to_device(po.scene(n, 11, K, 0.3, 0.5)[0]).reshape(1, n, 5)

    def single():
        ws = device.PnPWorkspace(1, n, h, dev)
        ws.run(view, K, THR, 10, RMS, philox=(77, 0, 1), solver="p3p")
        refined = ws.refine(view, K, THR, RMS, rounds=2)
        return [t.clone() for t in (ws.S, ws.model, ws.flags, ws.cnt, ws.s1, ws.s2, ws.result, ws.mask) + tuple(refined)]
    before = single()
    V, N = len(rv.SIZES), len(ragged["pts"])
    ws = _prefilled(V, N, h, dev)
    args = (ragged["pts_t"], ragged["offset_t"], ragged["min_extra_t"])
    ws.run(*args, K, THR, RMS, SEED, STRIDE, H_BEGIN, ROUNDS, MAX_STEPS)
    after = single()
    for a, b in zip(before, after):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    op = ops.load()
    Kl = [float(x) for x in K.reshape(9)]
    seed = device._as_int64(SEED)
    tail = (Kl, seed, STRIDE, H_BEGIN)
    pose, mask_out, info, status, mask, result = op.register_views(*args, *tail, h, THR, RMS, ROUNDS, MAX_STEPS)
    for got, name in ((pose, "pose_out"), (mask_out, "mask_out"), (info, "info"), (status, "status"), (mask, "mask"), (result, "result")):
        assert got.cpu().numpy().tobytes() == getattr(ws, name).cpu().numpy().tobytes(), name
    tests = ("test_schema", "test_faketensor")
    torch.library.opcheck(op.register_views.default, args + tail + (9, THR, RMS, ROUNDS, MAX_STEPS), test_utils=tests)
    small = device.RegisterViewsWorkspace(V, N, 9, dev)
    torch.library.opcheck(op.register_views_.default, args + tail + (THR, RMS, ROUNDS, MAX_STEPS) + small.buffers(), test_utils=tests)


# The margins of the app comparison: the sequential route's own spread over five Philox seeds on this scene, measured on an
# MI355X (profiles/register_views/README.md) — below the 2e-3 rad and 2e-2 that tests/test_gpu_view_graph.py::test_app_batched_route
# allows for the same kind of comparison, which are therefore the margins here.
ROTATION_MARGIN, TRANSLATION_MARGIN = 2e-3, 2e-2


def test_app_batched_route(dev):
    """Eight views: the batched route registers them all in fewer rounds than views, and its largest pose errors are the
    sequential P3P route's plus at most the margins."""
    from apps import sfm_multi_view

    sequential = sfm_multi_view.run(views=8, pnp_solver="p3p")
    batched = sfm_multi_view.run(views=8, register="batched")
    assert sequential["views_registered"] == 8 and batched["views_registered"] == 8
    rounds = batched["registration_rounds"]
    # fewer rounds than views; in fact fewer than the six registrations the sequential route makes behind the seed pair
    assert rounds["solver"] == "p3p" and 1 <= rounds["rounds"] < 6 and sum(rounds["views_per_round"]) == 6
    assert sorted(batched["registration_order"]) == list(range(8))
    worst = {name: (max(sequential[name].values()), max(batched[name].values())) for name in ("rotation_error_rad", "translation_error")}
    print("app routes (sequential, batched):", worst, rounds)
    assert worst["rotation_error_rad"][1] <= worst["rotation_error_rad"][0] + ROTATION_MARGIN
    assert worst["translation_error"][1] <= worst["translation_error"][0] + TRANSLATION_MARGIN
