"""Rotation and translation averaging on the GPU where tests/test_gpu_rotation_averaging.py and
tests/test_gpu_translation_averaging.py do not go: the logarithm against a definition of its own next to the half turn, the
shared core (csrc/sfm_graph_cg.h) beyond one scan tile, one stride of partials and one round of the grid-stride loops, the
strided NaN fillers, a CG cut at its limit, ``CG_FAILED``, and a side stream.

Bounds, all measured on the CPU:

* The logarithm: ``so3_log_cases.BOUND`` = 1.91e-13 rad, 1 000 x what half an ulp in one entry of D moves a 60-digit logarithm
  (1.91e-16 rad; tests/test_so3_log_host.py).
* The large graphs: 1 000 x the spread of tests/graph_cg_vector_oracle.py at each size, capped at 1e-8.  The spread is the
  largest difference among its float64 run, its 80-bit ``longdouble`` run and a run whose every solve stops one CG iteration
  earlier (rotations as angles and residuals in radians; positions in tree baselines, residuals in radians and scales):

      cameras     rotation (squared, Huber)    translation
        4 097     3.11e-16, 6.83e-15           3.56e-12
       65 537     2.10e-15, 4.22e-14           4.15e-11
      263 000     4.60e-15, 5.77e-14           1.15e-10

  kept as ``graph_cg_vector_oracle.LARGE_SPREAD`` per solver, size and loss (tests/test_graph_cg_vector_oracle_host.py measures
  the three at 4 097 cameras again); the translation bounds at the two larger sizes are the cap.  Rotations, residuals, positions
  and scales are all held to that one bound.
  One float64 run at 263 000 cameras takes 8 to 35 s of one CPU core, depending on the host (63 to 117 CG iterations per solve).
* Everything else: ``TOL`` of the two older files (3.55e-13 rad; 1.52e-9).
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import graph_cg_vector_oracle as vo
import rotation_averaging_oracle as ro
import so3_log_cases as sc
import translation_averaging_oracle as to
from test_gpu_rotation_averaging import TOL as ROT_TOL
from test_gpu_translation_averaging import TOL as TRANS_TOL

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def dev(native_lib):
    from structure_from_motion_amd import device

    return device.require_gpu()


def _rotations(case, initial=None, loss="squared", loss_scale=np.radians(1.0), **limits):
    """``device.average_rotations`` on a case dict -> the outputs on the host (residual in radians) and the info record."""
    from structure_from_motion_amd import device

    R, reg, level, residual, info = device.average_rotations(
        device.to_device(case["pairs"].astype(np.int32), torch.int32), device.to_device(case["relative"]),
        device.to_device(case["weights"]), case["C"], case.get("root", 0), None if initial is None else device.to_device(initial),
        loss, loss_scale, **limits)
    return SimpleNamespace(R=R.cpu().numpy(), registered=reg.cpu().numpy().astype(bool), level=level.cpu().numpy().astype(np.int64),
                           residual=residual.cpu().numpy(), info=device.read_rotavg_info(info), tensors=(R, reg, level, residual, info))


def _translations(case, initial=None, loss="squared", loss_scale=to.HUBER_SCALE, **limits):
    from structure_from_motion_amd import device

    c, reg, level, residual, scale, info = device.average_translations(
        device.to_device(case["pairs"].astype(np.int32), torch.int32), device.to_device(case["directions"]),
        device.to_device(case["weights"]), case["C"], case.get("root", 0), None, None if initial is None else device.to_device(initial),
        loss, loss_scale, **limits)
    return SimpleNamespace(c=c.cpu().numpy(), registered=reg.cpu().numpy().astype(bool), level=level.cpu().numpy().astype(np.int64),
                           residual=residual.cpu().numpy(), scale=scale.cpu().numpy(), info=device.read_transavg_info(info),
                           tensors=(c, reg, level, residual, scale, info))


def _same_record(got, want, where, counters=True):
    """registered, level, steps, status, rounds (and the CG counters) equal; the costs within 1e-9 relative."""
    assert np.array_equal(got.registered, want["registered"]) and np.array_equal(got.level, want["level"]), where
    rec = got.info
    assert (rec.status, rec.steps) == (want["status"], want["steps"]), (where, rec, want["status"], want["steps"])
    assert rec.registered == int(want["registered"].sum()) and rec.rounds == max(int(want["level"].max()), 0), (where, rec)
    if counters:
        assert (rec.cg_iterations, rec.cg_max) == (want["cg_iterations"], want["cg_max"]), (where, rec, want["cg_iterations"])
    for a, b in ((rec.initial_cost, want["initial_cost"]), (rec.final_cost, want["final_cost"])):
        assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-9 * max(abs(b), 1e-12), (where, a, b)


def _rotation_values(got, want, tol, where, residual_tol=None):
    """``residual_tol``: 2 x tol where tol is the older files' ``TOL`` for a rotation (a residual sees the rotations of both
    ends, as there); tol itself for the large graphs, whose spread is measured over rotations and residuals alike."""
    residual_tol = 2 * tol if residual_tol is None else residual_tol
    reg, used = want["registered"], ~np.isnan(want["residual"])
    assert np.array_equal(np.isnan(got.residual), ~used) and np.isnan(got.R[~reg]).all() and np.isfinite(got.R[reg]).all(), where
    diff = float(np.max(vo.rotation_angles(got.R[reg], want["R"][reg])))
    res = float(np.max(np.abs(got.residual[used] - want["residual"][used]))) if used.any() else 0.0
    print(f"{where}: steps {got.info.steps} cg {got.info.cg_iterations} (most {got.info.cg_max}); rotations differ by {diff:.3g} rad, "
          f"residuals by {res:.3g} rad (tolerance {tol:.3g}); cost {got.info.initial_cost:.6g} -> {got.info.final_cost:.6g}")
    assert diff <= tol and res <= residual_tol, (where, diff, res, tol, residual_tol)


def _translation_values(got, want, tol, where):
    reg, used = want["registered"], ~np.isnan(want["residual"])
    assert np.array_equal(np.isnan(got.residual), ~used) and np.array_equal(np.isnan(got.scale), ~used), where
    assert np.isnan(got.c[~reg]).all() and np.isfinite(got.c[reg]).all(), where
    pos = float(np.max(np.abs(got.c[reg] - want["c"][reg])))
    res = float(np.max(np.abs(got.residual[used] - want["residual"][used]))) if used.any() else 0.0
    scale = float(np.max(np.abs(got.scale[used] - want["scale"][used]))) if used.any() else 0.0
    print(f"{where}: steps {got.info.steps} cg {got.info.cg_iterations} (most {got.info.cg_max}); positions differ by {pos:.3g}, "
          f"residuals by {res:.3g} rad, scales by {scale:.3g} (tolerance {tol:.3g}); cost {got.info.initial_cost:.6g} -> "
          f"{got.info.final_cost:.6g}")
    assert pos <= tol and res <= tol and scale <= tol, (where, pos, res, scale, tol)


# ---- 1. the logarithm on a star --------------------------------------------------------------------------------------------------
def test_logarithm_on_a_star(dev):
    """One edge (0, k) or (k, 0) per rotation of the sweep of tests/so3_log_cases.py, every camera started at the identity: D of
    edge k is its rotation bit for bit, the Laplacian of a star is diagonal, and one step with one CG iteration leaves
    R_k = exp(+-log R_q).  Measured on an MI355X: R_k is off R_q by at most 1.96e-15 rad, and the residuals without a step off
    the angles by 1.33e-15 rad.  With the logarithm before (v theta / s down to s = 1e-10) R_k was off by 8.71e-7 rad at
    pi - 1e-10, 1.2e-13 at pi - 1e-3 and above the bound from pi - 1e-5 on (1.0e-11 rad there); the residuals, which see the
    angle alone, were as good as now."""
    sweep = sc.sweep()
    n = len(sweep)
    rel = np.array([D for _, D, _, _ in sweep])
    truth = np.array([np.linalg.norm(r) for _, _, r, _ in sweep])
    pairs = np.array([(0, k) if k % 2 else (k, 0) for k in range(1, n + 1)])
    case = dict(C=n + 1, pairs=pairs, relative=rel, weights=np.ones(n), root=0)
    start = np.tile(np.eye(3), (n + 1, 1, 1))
    want_R = np.where((pairs[:, 0] == 0)[:, None, None], rel, np.swapaxes(rel, 1, 2))
    # no step: the residual is the angle, the cost the sum of the squared angles
    still = _rotations(case, initial=start, max_steps=0)
    worst = int(np.argmax(np.abs(still.residual - truth)))
    print(f"star, no step: residuals differ from the angles by at most {abs(still.residual[worst] - truth[worst]):.3g} rad "
          f"({sweep[worst][0]})")
    assert np.max(np.abs(still.residual - truth)) <= sc.BOUND
    assert still.info.initial_cost == still.info.final_cost
    assert abs(still.info.initial_cost - float(np.sum(truth * truth))) <= 2 * np.pi * sc.BOUND * n
    assert np.array_equal(still.R, start) and still.info.status == ro.MAX_STEPS and still.info.steps == 0
    _same_record(still, ro.average_rotations(n + 1, pairs, rel, initial_rotations=start, max_steps=0), "star, no step")
    # one step
    moved = _rotations(case, initial=start, max_steps=1)
    err = vo.rotation_angles(moved.R[1:], want_R)
    worst = int(np.argmax(err))
    print(f"star, one step: exp(log R) is off R by at most {err[worst]:.3g} rad ({sweep[worst][0]}); cg {moved.info.cg_iterations}")
    by_angle = {}
    for (name, _, _, _), e in zip(sweep, err):
        angle = name.split(" at ")[1]
        by_angle[angle] = max(by_angle.get(angle, 0.0), float(e))
    print("   by angle:", ", ".join(f"{a}: {e:.2g}" for a, e in by_angle.items()))
    assert moved.info.cg_iterations == 1 and moved.info.steps == 1
    assert err.max() <= sc.BOUND
    want = ro.average_rotations(n + 1, pairs, rel, initial_rotations=start, max_steps=1)
    _same_record(moved, want, "star, one step")
    _rotation_values(moved, want, ROT_TOL, "star, one step")


# ---- 2. beyond one tile, one stride, one block of partials ------------------------------------------------------------------------
LARGE_LOSSES = {"rotation": ("squared", "huber"), "translation": ("squared",)}


@pytest.fixture(scope="module")
def large_cases():
    """Every large case and the vector oracle's float64 result of it, computed once per size and solver."""
    made = {}

    def get(solver, cameras, loss):
        if (solver, cameras) not in made:
            made[solver, cameras] = vo.large_case(solver, cameras)
        if (solver, cameras, loss) not in made:
            made[solver, cameras, loss] = vo.large_run(solver, made[solver, cameras], loss)
        return made[solver, cameras], made[solver, cameras, loss]

    return get


def _large_checks(case, got, want, cameras):
    """What the sizes are for: more than one scan tile, 256 CG blocks, one grid-stride round, 1 024 cost partials."""
    Q = len(case["pairs"])
    assert Q == 3 * cameras - (1 if cameras < 262144 else 2) and 5 <= got.info.rounds <= 16
    if cameras < 262144:
        assert got.registered.all()
        return
    assert Q > 1024 * 256 and case["root"] == cameras - 1 and got.level[cameras - 1] == 0
    cut = np.arange(cameras - 1 - vo.CUT, cameras - 1)
    assert not got.registered[cut].any() and got.registered.sum() == cameras - vo.CUT and (got.level[cut] == -1).all()
    at_cut = np.isin(case["pairs"], cut).any(axis=1)
    assert at_cut.sum() == 3 * vo.CUT - 1 and np.isnan(got.residual[at_cut]).all() and np.isnan(got.residual[case["switched_off"]]).all()
    assert np.isnan(got.residual).sum() == at_cut.sum() + len(case["switched_off"])


@pytest.mark.parametrize("loss", LARGE_LOSSES["rotation"])
@pytest.mark.parametrize("cameras", vo.LARGE_SIZES)
def test_large_rotation_graph(dev, large_cases, cameras, loss):
    case, want = large_cases("rotation", cameras, loss)
    got = _rotations(case, loss=loss, **vo.LARGE_LIMITS)
    where = f"rotation, {cameras} cameras, {loss}"
    _large_checks(case, got, want, cameras)
    _same_record(got, want, where, counters=False)   # a CG that stops at its tolerance may stop an iteration apart
    assert abs(got.info.cg_iterations - want["cg_iterations"]) <= want["steps"] and got.info.status == ro.MAX_STEPS
    tol = min(1000 * vo.LARGE_SPREAD["rotation", cameras, loss], 1e-8)
    _rotation_values(got, want, tol, where, residual_tol=tol)
    if cameras > 262144:
        assert np.isnan(got.R[~got.registered]).all() and np.array_equal(got.R[cameras - 1], np.eye(3))


@pytest.mark.parametrize("cameras", vo.LARGE_SIZES)
def test_large_translation_graph(dev, large_cases, cameras):
    case, want = large_cases("translation", cameras, "squared")
    got = _translations(case, warmup_steps=1, **vo.LARGE_LIMITS)
    where = f"translation, {cameras} cameras"
    _large_checks(case, got, want, cameras)
    _same_record(got, want, where, counters=False)
    assert abs(got.info.cg_iterations - want["cg_iterations"]) <= want["steps"] and got.info.status == to.MAX_STEPS
    _translation_values(got, want, min(1000 * vo.LARGE_SPREAD["translation", cameras, "squared"], 1e-8), where)
    if cameras > 262144:
        assert np.isnan(got.c[~got.registered]).all() and np.array_equal(got.c[cameras - 1], np.zeros(3))
        assert np.isnan(got.scale[case["switched_off"]]).all()


@pytest.mark.parametrize("solver", ["rotation", "translation", "translation with rotations"])
def test_bad_index_last_fills_every_output_in_strides(dev, native_lib, solver):
    """3 000 cameras and 5 000 edges, the bad pair last: every filler of the finish kernels goes round its 1 024 threads more
    than once, after every other kernel has seen 4 999 good edges."""
    from structure_from_motion_amd import _native, device

    C, Q, guard = 3000, 5000, 64
    pairs, weights, _, rng = vo.large_graph(C, 15)
    pairs = pairs[:Q].astype(np.int32)
    pairs[-1] = (C - 1, C)
    lib = native_lib
    rotation = solver == "rotation"
    bytes_ = (lib.sfm_average_rotations_workspace_bytes if rotation else lib.sfm_average_translations_workspace_bytes)(C, Q)
    ws = torch.zeros(bytes_ + guard, dtype=torch.uint8, device=dev)
    ws[bytes_:] = 0xA5
    width = 9 if rotation else 3
    main = torch.full((width * C + guard,), 7.0, dtype=torch.float64, device=dev)
    reg = torch.full((C + guard,), 9, dtype=torch.uint8, device=dev)
    level = torch.full((C + guard,), 77, dtype=torch.int32, device=dev)
    residual = torch.full((Q + guard,), 7.0, dtype=torch.float64, device=dev)
    scale = torch.full((Q + guard,), 7.0, dtype=torch.float64, device=dev)
    info = torch.full((5 + guard,), 123, dtype=torch.int64, device=dev)
    p, w = device.to_device(pairs, torch.int32), device.to_device(weights[:Q])
    rot = device.to_device(vo.exp_map(rng.normal(size=(max(C, Q), 3))))
    if rotation:
        opts = _native.RotavgOptions(0, _native.ROTAVG_INIT_TREE, 10, 50, 1.0, 1e-6, 1e-8)
        rc = lib.sfm_average_rotations(C, Q, p.data_ptr(), rot.data_ptr(), w.data_ptr(), 0, None, ctypes.byref(opts), main.data_ptr(),
                                       reg.data_ptr(), level.data_ptr(), residual.data_ptr(), info.data_ptr(), ws.data_ptr(), bytes_,
                                       None)
    else:
        opts = _native.TransavgOptions(0, _native.TRANSAVG_INIT_TREE, 10, 50, 2, 0, 0.03, 1e-6, 1e-8)
        d = device.to_device(to.unit(rng.normal(size=(Q, 3))))
        rc = lib.sfm_average_translations(C, Q, p.data_ptr(), d.data_ptr(), rot.data_ptr() if "with" in solver else None, w.data_ptr(),
                                          0, None, ctypes.byref(opts), main.data_ptr(), reg.data_ptr(), level.data_ptr(),
                                          residual.data_ptr(), scale.data_ptr(), info.data_ptr(), ws.data_ptr(), bytes_, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.sfm_last_error()
    rec = device.read_graph_info(info[:5])
    assert rec.status == device.ROTAVG_BAD_INDEX and rec.steps == 0 and rec.registered == 0 and rec.cg_iterations == 0
    assert rec.cg_max == 0 and rec.rounds == 0 and np.isnan(rec.initial_cost) and np.isnan(rec.final_cost)
    assert torch.isnan(main[:width * C]).all() and torch.isnan(residual[:Q]).all()
    assert (reg[:C] == 0).all() and (level[:C] == -1).all()
    assert (main[width * C:] == 7.0).all() and (residual[Q:] == 7.0).all() and (reg[C:] == 9).all() and (level[C:] == 77).all()
    assert (info[5:] == 123).all() and (ws[bytes_:] == 0xA5).all()
    if rotation:
        assert (scale == 7.0).all()
    else:
        assert torch.isnan(scale[:Q]).all() and (scale[Q:] == 7.0).all()


# ---- 3. statuses, counters and streams ---------------------------------------------------------------------------------------------
def _ring(solver):
    """40 cameras on a ring with 80 chords, 0.5 degrees of noise."""
    if solver == "rotation":
        g = ro.make_graph(40, 80, 31, noise_deg=0.5)
        return dict(C=40, pairs=g["pairs"], relative=g["relative"], weights=np.ones(120), root=0)
    g = to.make_graph(40, 80, 31, noise_deg=0.5)
    return dict(C=40, pairs=g["pairs"], directions=g["directions"], weights=np.ones(120), root=0)


CUT_LIMITS = dict(max_steps=3, step_tolerance=1e-300, cg_tolerance=1e-15)


@pytest.mark.parametrize("limit", [1, 9, 10, 11, 20, 21])
def test_cg_cut_at_its_limit(dev, limit):
    """cg_tolerance = 1e-15 is out of reach of 21 iterations on this graph (with room the oracle's longest solve takes 34
    iterations for the rotations and 36 for the positions), so every solve ends at ``max_cg_iterations``: inside the host's
    chunk of 10, at its end, and in the chunks after it.  The public functions and the ``_assert_matches`` of the two older
    files see the same runs."""
    import test_gpu_rotation_averaging as tr
    import test_gpu_translation_averaging as tt

    for solver in ("rotation", "translation"):
        case = _ring(solver)
        if solver == "rotation":
            want = ro.average_rotations(40, case["pairs"], case["relative"], max_cg_iterations=limit, **CUT_LIMITS)
            got = _rotations(case, max_cg_iterations=limit, **CUT_LIMITS)
        else:
            want = to.average_translations(40, case["pairs"], case["directions"], warmup_steps=1, max_cg_iterations=limit, **CUT_LIMITS)
            got = _translations(case, warmup_steps=1, max_cg_iterations=limit, **CUT_LIMITS)
        where = f"{solver}, CG cut at {limit}"
        assert want["steps"] == 3 and want["cg_max"] == limit and want["cg_iterations"] == 3 * limit, (where, want["cg_iterations"])
        assert got.info.cg_max == limit and got.info.cg_iterations == got.info.steps * limit and got.info.steps == 3, (where, got.info)
        _same_record(got, want, where)
        (_rotation_values if solver == "rotation" else _translation_values)(got, want, ROT_TOL if solver == "rotation" else TRANS_TOL,
                                                                            where)
        if solver == "rotation":
            public = tr._device(case, max_cg_iterations=limit, **CUT_LIMITS)
            tr._assert_matches(public, want, where)
        else:
            public = tt._device(case, warmup_steps=1, max_cg_iterations=limit, **CUT_LIMITS)
            tt._assert_matches(public, want, where)
        assert want["cg_at_limit"] and public.cg_iterations == 3 * limit, where   # so _assert_matches compared the counter


def _raw(dev, native_lib, solver, case, initial, max_steps, warmup_steps=0, cg_tolerance=1e-12, guard=64):
    """``sfm_average_rotations`` or ``sfm_average_translations`` through the C ABI with a pattern in, and a guard behind, every
    output and the workspace -> the outputs on the host, after checking that every guard is intact and every pattern gone."""
    from structure_from_motion_amd import _native, device

    lib, C, Q = native_lib, case["C"], len(case["pairs"])
    rotation = solver == "rotation"
    bytes_ = (lib.sfm_average_rotations_workspace_bytes if rotation else lib.sfm_average_translations_workspace_bytes)(C, Q)
    ws = torch.zeros(bytes_ + guard, dtype=torch.uint8, device=dev)
    ws[bytes_:] = 0xA5
    width = 9 if rotation else 3
    main = torch.full((width * C + guard,), 7.0, dtype=torch.float64, device=dev)
    reg = torch.full((C + guard,), 9, dtype=torch.uint8, device=dev)
    level = torch.full((C + guard,), 77, dtype=torch.int32, device=dev)
    residual = torch.full((Q + guard,), 7.0, dtype=torch.float64, device=dev)
    scale = torch.full((Q + guard,), 7.0, dtype=torch.float64, device=dev)
    info = torch.full((5 + guard,), 123, dtype=torch.int64, device=dev)
    p, w = device.to_device(case["pairs"].astype(np.int32), torch.int32), device.to_device(case["weights"])
    init = None if initial is None else device.to_device(initial)
    start = _native.ROTAVG_INIT_TREE if initial is None else _native.ROTAVG_INIT_GIVEN
    if rotation:
        opts = _native.RotavgOptions(0, start, max_steps, 500, np.radians(1.0), cg_tolerance, 1e-8)
        rel = device.to_device(case["relative"])
        rc = lib.sfm_average_rotations(C, Q, p.data_ptr(), rel.data_ptr(), w.data_ptr(), case["root"],
                                       None if init is None else init.data_ptr(), ctypes.byref(opts), main.data_ptr(), reg.data_ptr(),
                                       level.data_ptr(), residual.data_ptr(), info.data_ptr(), ws.data_ptr(), bytes_, None)
    else:
        opts = _native.TransavgOptions(0, start, max_steps, 500, warmup_steps, 0, to.HUBER_SCALE, cg_tolerance, 1e-8)
        d = device.to_device(case["directions"])
        rc = lib.sfm_average_translations(C, Q, p.data_ptr(), d.data_ptr(), None, w.data_ptr(), case["root"],
                                          None if init is None else init.data_ptr(), ctypes.byref(opts), main.data_ptr(),
                                          reg.data_ptr(), level.data_ptr(), residual.data_ptr(), scale.data_ptr(), info.data_ptr(),
                                          ws.data_ptr(), bytes_, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.sfm_last_error()
    assert (main[width * C:] == 7.0).all() and (reg[C:] == 9).all() and (level[C:] == 77).all() and (residual[Q:] == 7.0).all()
    assert (info[5:] == 123).all() and (ws[bytes_:] == 0xA5).all() and (scale[Q if not rotation else 0:] == 7.0).all()
    got = SimpleNamespace(registered=reg[:C].cpu().numpy().astype(bool), level=level[:C].cpu().numpy().astype(np.int64),
                          residual=residual[:Q].cpu().numpy(), info=device.read_graph_info(info[:5]))
    values = main[:width * C].cpu().numpy()
    if rotation:
        got.R = values.reshape(C, 3, 3)
    else:
        got.c, got.scale = values.reshape(C, 3), scale[:Q].cpu().numpy()
        assert not np.any(got.scale == 7.0)
    # every byte written: the patterns are gone
    assert not np.any(values == 7.0) and not np.any(got.residual == 7.0) and not np.any(got.level == 77)
    assert set(np.unique(reg[:C].cpu().numpy())) <= {0, 1}
    return got


def test_cg_failed_rotation(dev, native_lib):
    """One NaN entry in the given rotation of a registered camera that is not the root: |b|^2 of the first step is NaN.  The
    oracle defines the result: the given rotations, NaN residuals at that camera's edges, NaN costs, no step."""
    case = _ring("rotation")
    tree = ro.average_rotations(40, case["pairs"], case["relative"], max_steps=0)
    initial = tree["R"].copy()
    initial[7, 1, 2] = np.nan
    want = ro.average_rotations(40, case["pairs"], case["relative"], initial_rotations=initial, max_steps=5, cg_tolerance=1e-12)
    assert want["status"] == ro.CG_FAILED and want["steps"] == 0 and want["cg_iterations"] == 0
    got = _raw(dev, native_lib, "rotation", case, initial, 5)
    assert ro.STATUS[got.info.status] == "cg_failed" and got.info.steps == 0
    _same_record(got, want, "rotation, CG_FAILED")
    assert np.array_equal(got.R, want["R"], equal_nan=True) and np.array_equal(got.R, initial, equal_nan=True)
    at7 = np.any(case["pairs"] == 7, axis=1)
    assert np.array_equal(np.isnan(got.residual), at7) and np.array_equal(np.isnan(want["residual"]), at7)
    assert np.max(np.abs(got.residual[~at7] - want["residual"][~at7])) <= 2 * ROT_TOL
    assert np.isnan(got.info.initial_cost) and np.isnan(got.info.final_cost) and got.registered.all()
    # the torch op returns the same bytes and the same status
    op = _rotations(case, initial=initial, max_steps=5, cg_tolerance=1e-12)
    assert ro.STATUS[op.info.status] == "cg_failed" and np.isnan(op.info.initial_cost) and np.isnan(op.info.final_cost)
    assert (op.info.steps, op.info.cg_iterations, op.info.cg_max, op.info.registered, op.info.rounds) == \
        (0, 0, 0, 40, got.info.rounds)
    for name in ("R", "registered", "level", "residual"):
        assert getattr(op, name).tobytes() == getattr(got, name).tobytes(), name


def test_cg_failed_translation_in_the_first_step(dev, native_lib):
    """Two chords of weight 1e200: their share of b is about 1e200, |b|^2 overflows, the first solve fails.  The result is
    the tree start."""
    case = _ring("translation")
    case["weights"] = case["weights"].copy()
    case["weights"][[50, 90]] = 1e200
    want = to.average_translations(40, case["pairs"], case["directions"], case["weights"], warmup_steps=2, max_steps=5,
                                   cg_tolerance=1e-12)
    assert want["status"] == to.CG_FAILED and want["steps"] == 0 and np.isfinite(want["initial_cost"])
    got = _raw(dev, native_lib, "translation", case, None, 5, warmup_steps=2)
    assert to.STATUS[got.info.status] == "cg_failed" and got.info.steps == 0
    _same_record(got, want, "translation, CG_FAILED in step 0")
    assert np.array_equal(got.c, want["c"])   # the tree start, bit for bit
    _translation_values(got, want, TRANS_TOL, "translation, CG_FAILED in step 0")


def test_cg_failed_translation_in_the_second_step(dev, native_lib):
    """Camera 40 hangs on the root by two edges alone, of weights W and 3 W (W = 2^665), directions e0 and e1, and is given the
    position (1/4, 3/4, 0).  In the warm-up step (every scale 1) the two terms W (e0 - D) and 3 W (e1 - D) cancel to the last
    bit, its row has a zero right-hand side and it stays; in the second step the scales are 0.4 and 1.2, the terms no longer
    cancel, |b|^2 overflows and the solve fails.  DESIGN.md §6t.3: the state of the last completed step, so the positions
    after the warm-up step."""
    base = _ring("translation")
    W = 2.0 ** 665
    case = dict(C=41, pairs=np.concatenate([base["pairs"], [(0, 40), (0, 40)]]),
                directions=np.concatenate([base["directions"], [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0)]]),
                weights=np.concatenate([base["weights"], [W, 3 * W]]), root=0)
    tree = to.average_translations(41, case["pairs"], case["directions"], case["weights"], max_steps=0)
    initial = tree["c"].copy()
    initial[40] = (0.25, 0.75, 0.0)
    kw = dict(initial_positions=initial, warmup_steps=1, cg_tolerance=1e-12)
    want = to.average_translations(41, case["pairs"], case["directions"], case["weights"], max_steps=4, **kw)
    one = to.average_translations(41, case["pairs"], case["directions"], case["weights"], max_steps=1, **kw)
    assert want["status"] == to.CG_FAILED and want["steps"] == 1 and want["cg_iterations"] == one["cg_iterations"] > 0
    assert np.array_equal(want["c"], one["c"]) and np.array_equal(want["c"][40], initial[40]) and not np.array_equal(want["c"], initial)
    got = _raw(dev, native_lib, "translation", case, initial, 4, warmup_steps=1)
    assert to.STATUS[got.info.status] == "cg_failed" and got.info.steps == 1
    _same_record(got, want, "translation, CG_FAILED in step 1", counters=False)
    assert abs(got.info.cg_iterations - want["cg_iterations"]) <= 1 and got.info.cg_max == got.info.cg_iterations
    assert np.array_equal(got.c[40], initial[40])
    _translation_values(got, want, TRANS_TOL, "translation, CG_FAILED in step 1")
    assert np.isfinite(got.info.initial_cost) and np.isfinite(got.info.final_cost)


def test_side_stream_same_bytes(dev):
    """The Huber case of ``case_losses`` on a side stream, with unrelated work queued on the default stream: the host loop reads
    its flags on the caller's stream."""
    rot, tra = ro.case_losses(), to.case_losses()
    rot_kw = dict(loss="huber", loss_scale=np.radians(1.0), max_steps=60, step_tolerance=1e-300, cg_tolerance=1e-10)
    tra_kw = dict(loss="huber", loss_scale=to.HUBER_SCALE, max_steps=20, warmup_steps=5, **to.FIXED)

    def both():
        return [t.cpu().numpy().tobytes() for t in _rotations(rot, **rot_kw).tensors + _translations(tra, **tra_kw).tensors]

    first = both()
    side = torch.cuda.Stream()
    busy = torch.randn(4096, 4096, device=dev)
    torch.cuda.synchronize()
    for _ in range(20):
        busy = busy @ busy * 1e-3   # on the default stream, still running when the side stream starts
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream() == side
        again = both()
    torch.cuda.synchronize()
    assert first == again and len(first) == 11
