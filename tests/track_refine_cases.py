"""Scenes, observation lists and pinned figures of the sub-pixel track refinement, shared by
tests/test_track_refine_host.py and tests/test_gpu_track_refine.py, and the stream case of its two entry points.

  analytic textures   a band-limited sum of sinusoids, quantised to uint8, rendered under a known shift or rotation: the position
                      error of the definition is known exactly
  accuracy scene      the four distinct views of similarity_texture_views(240, 320, ...) with keypoint_oracle keypoints and
                      graph_matching_oracle matches against view 0: real orientation bins, real matches
  device collection   three images of 48 x 48, 60 x 75 (two levels) and 97 x 131 (three levels) of one analytic texture under an
                      identity, a quarter turn and an anisotropic map, with a constant block and a checkerboard block painted into
                      the third; observation lists of any length with every kind of reference, warp and status
"""
import functools

import numpy as np

import keypoint_oracle as ko
import stream_cases
import track_refine_oracle as tro

F = np.float64

# ---- analytic textures ---------------------------------------------------------------------------------------------------------
# (fx, fy, phase, amplitude) in cycles per pixel: wavelengths of 7 to 31 pixels
_WAVES = ((0.061, 0.023, 0.3, 1.0), (-0.034, 0.071, 1.1, 0.9), (0.093, -0.047, 2.0, 0.7), (0.017, 0.102, 0.7, 0.8),
          (0.128, 0.064, 2.6, 0.5), (-0.081, -0.119, 1.7, 0.5), (0.142, -0.012, 0.2, 0.4), (0.032, 0.033, 2.9, 1.1))


def texture_value(X, Y, seed=0):
    """The texture at canvas points, 0 .. 255 before quantisation; ``seed`` shifts every phase."""
    total = np.zeros(np.broadcast(X, Y).shape)
    for k, (fx, fy, phase, amplitude) in enumerate(_WAVES):
        total = total + amplitude * np.sin(2.0 * np.pi * (fx * X + fy * Y) + phase + 1.37 * seed * (k + 1))
    return 127.5 + 127.5 * total / sum(w[3] for w in _WAVES)


def render(height, width, A, seed=0):
    """uint8 [height, width]: pixel (x, y) shows the texture at canvas point A @ (x, y, 1), A float64 [2, 3]."""
    x, y = np.meshgrid(np.arange(width, dtype=F), np.arange(height, dtype=F))
    A = np.asarray(A, dtype=F)
    value = texture_value(A[0, 0] * x + A[0, 1] * y + A[0, 2], A[1, 0] * x + A[1, 1] * y + A[1, 2], seed)
    return np.clip(np.floor(value + 0.5), 0, 255).astype(np.uint8)


def rotation(degrees):
    a = np.deg2rad(degrees)
    return np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])


SHIFT = (0.37, -0.21)             # the second rendering shows the texture this much further right / up
SHIFT_INTEGER_ERROR = 0.43        # |SHIFT|: how far the integer position is off (0.4254)
SIDE, CENTRE = 64, 32


def shift_case():
    """(reference image, shifted image, true position of the reference's pixel (CENTRE, CENTRE) in the shifted image)."""
    identity = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    moved = np.array([[1.0, 0.0, -SHIFT[0]], [0.0, 1.0, -SHIFT[1]]])
    return render(SIDE, SIDE, identity), render(SIDE, SIDE, moved), (CENTRE + SHIFT[0], CENTRE + SHIFT[1])


def rotation_case(degrees=10.0, start_off=6.0):
    """The same with the second image also rotated by ``degrees`` about the shifted point; warp0 is ``start_off`` degrees off."""
    R = rotation(degrees)
    truth = np.array([CENTRE + SHIFT[0], CENTRE + SHIFT[1]])
    # canvas = R^-1 (p - truth) + (CENTRE, CENTRE): window offsets d of the reference appear at truth + R d
    Rinv = R.T
    A = np.column_stack([Rinv, np.array([CENTRE, CENTRE]) - Rinv @ truth])
    identity = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    return render(SIDE, SIDE, identity), render(SIDE, SIDE, A), tuple(truth), rotation(degrees + start_off).reshape(4)


def position_error(result, truth):
    return float(np.hypot(result[1][0] - truth[0], result[1][1] - truth[1]))


# the definition's position error on the two cases at the defaults (radius 7, 10 iterations), measured once with the oracle and
# pinned to 1e-9 by the host test; the issue's condition is a quarter of SHIFT_INTEGER_ERROR
SHIFT_ERROR = 0.010846872715228278      # 4 solves, correlation 0.99967
ROTATION_ERROR = 0.015765200668300644   # 5 solves, correlation 0.99971


# ---- the accuracy scene -----------------------------------------------------------------------------------------------------------
ACCURACY_VIEWS = (1, 2, 4)        # each against view 0 (view 3 repeats view 0)


def _canvas(A, xy):
    return xy @ A[:, :2].T + A[:, 2]


@functools.lru_cache(maxsize=None)
def accuracy_scene():
    """Per second view v: dict(before, after [pairs] canvas distances, status [pairs]) of the right matches of
    graph_matching_oracle.match_pair at its defaults between view 0 and view v, refined by the definition at its defaults with
    view 0's end as the reference and warp0 from the two orientation bins."""
    import graph_matching_oracle as gm
    from structure_from_motion_amd import synthetic
    from structure_from_motion_amd.multiview import track_refinement as tr

    degrees, scales = (0, 17, 45, 0, 133), (1, 1.25, 1.5, 1, 2)
    images, to_canvas = synthetic.similarity_texture_views(240, 320, degrees, scales, seed=7)
    maps = [ko.Maps(image, 8, 20) for image in images]
    keypoints = [ko.describe(m, 1000) for m in maps]
    out = {}
    for v in ACCURACY_VIEWS:
        a, b = keypoints[0], keypoints[v]
        partner, _ = gm.match_pair(a.bits, a.valid, b.bits, b.valid)
        ia = np.nonzero(partner >= 0)[0]
        ib = partner[ia].astype(np.int64)
        ca = _canvas(to_canvas[0], a.xy[ia])
        apart = np.linalg.norm(ca - _canvas(to_canvas[v], b.xy[ib]), axis=1)
        footprint = np.maximum(scales[0] * 1.25 ** a.level[ia].astype(F), scales[v] * 1.25 ** b.level[ib].astype(F))
        right = apart <= 3.0 * footprint                    # section 6x's rule
        ia, ib, ca = ia[right], ib[right], ca[right]
        n = len(ia)
        planes = maps[0].planes + maps[v].planes
        plane = np.concatenate([a.level[ia].astype(np.int64), len(maps[0].planes) + b.level[ib].astype(np.int64)])
        x, y = np.concatenate([a.level_xy[ia, 0], b.level_xy[ib, 0]]), np.concatenate([a.level_xy[ia, 1], b.level_xy[ib, 1]])
        reference = np.concatenate([np.full(n, -1), np.arange(n)])
        warp0 = np.concatenate([np.tile([1.0, 0.0, 0.0, 1.0], (n, 1)), tr.bin_rotation(a.angle_bin[ia], b.angle_bin[ib])])
        result = tro.refine(planes, plane, x, y, reference, warp0)
        after = np.linalg.norm(ca - _canvas(to_canvas[v], ko.base_xy(result.xy[n:, 0], result.xy[n:, 1], b.level[ib])), axis=1)
        out[v] = dict(before=apart[right], after=after, status=result.status[n:].copy(), iterations=result.iterations[n:].copy())
    return out


# view -> (pairs, median before, median after, pairs left unrefined), the definition's figures, pinned by the host test
ACCURACY = {1: (352, 0.9264864932375014, 0.04762621012125968, 0), 2: (173, 1.0196958222144672, 0.050231654886978214, 0),
            4: (93, 1.2131284079072724, 0.05932493332470361, 0)}


# ---- the device collection ----------------------------------------------------------------------------------------------------------
SHAPES = ((48, 48), (60, 75), (97, 131))
LEVELS = 3
CANVAS_CENTRE = np.array([200.0, 200.0])
# image pixel (x, y) -> canvas: centre + L (p - image centre); an identity, a quarter turn and an anisotropic map with shear
LINEAR = (np.eye(2), rotation(90.0), np.array([[1.10, 0.07], [-0.04, 0.92]]))
FLAT_BLOCK = (0, 0, 21)           # (x, y, side) in image 2: constant grey
CHECKER_BLOCK = (110, 76, 21)     # in image 2: a one-pixel checkerboard, whose central differences all vanish


def to_canvas_map(i):
    h, w = SHAPES[i]
    centre = np.array([(w - 1) / 2.0, (h - 1) / 2.0])
    return np.column_stack([LINEAR[i], CANVAS_CENTRE - LINEAR[i] @ centre])


@functools.lru_cache(maxsize=None)
def collection(seed=0):
    """(images, rows, planes): the three uint8 images, the plane table rows (image, level, height, width, offset, quota) in the
    pool's order and the definition's planes in that order."""
    from structure_from_motion_amd.feature_matching import keypoints as kp

    images = [render(h, w, to_canvas_map(i), seed) for i, (h, w) in enumerate(SHAPES)]
    x, y, side = FLAT_BLOCK
    images[2][y:y + side, x:x + side] = 90 + 40 * seed
    x, y, side = CHECKER_BLOCK
    yy, xx = np.mgrid[0:side, 0:side]
    images[2][y:y + side, x:x + side] = np.where((xx + yy) % 2 == 0, 40, 200 - 30 * seed)
    rows = kp.plan(SHAPES, 1, LEVELS).rows
    pyramids = [ko.pyramid(image, LEVELS) for image in images]
    planes = [pyramids[row[0]][row[1]] for row in rows]
    assert [len(p) for p in pyramids] == [1, 2, 3] and [p.shape for p in planes] == [(r[2], r[3]) for r in rows]
    return images, rows, planes


def plane_index(rows, image, level):
    return [(r[0], r[1]) for r in rows].index((image, level))


def _level_to_canvas(i, level):
    """[2, 3]: pixel of level ``level`` of image i -> canvas."""
    A, s = to_canvas_map(i), 1.25 ** level
    return np.column_stack([A[:, :2] * s, A[:, :2] @ np.array([0.5 * s - 0.5, 0.5 * s - 0.5]) + A[:, 2]])


_SLOTS = ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2))   # (image, level) of every plane


def observations(M, seed=1, permute=False, warp_noise=0.02):
    """An observation list of length M on the device collection: tracks of two to four observations of one canvas point each, the
    first one the reference, on planes drawn at random (other images, other levels of the same image, the same plane twice);
    warp0 is the true linear map between the two planes, perturbed a little.  ``permute``: the list in a random order, so that
    references point forwards as well as backwards.  -> dict(plane, x, y, reference, warp0)."""
    _, rows, planes = collection()
    rng = np.random.default_rng(seed)
    plane, x, y, reference, warp0 = [], [], [], [], []
    while len(plane) < M:
        point = CANVAS_CENTRE + rng.uniform(-11.0, 11.0, 2)
        length = int(rng.integers(2, 5))
        first = len(plane)
        for k in range(length):
            i, level = _SLOTS[int(rng.integers(0, len(_SLOTS)))]
            A = _level_to_canvas(i, level)
            p = np.linalg.solve(A[:, :2], point - A[:, 2])
            plane.append(plane_index(rows, i, level))
            x.append(int(np.rint(p[0])))
            y.append(int(np.rint(p[1])))
            reference.append(-1 if k == 0 else first)
            if k == 0:
                first_map = A[:, :2]
                warp0.append([1.0, 0.0, 0.0, 1.0])
            else:
                warp0.append((np.linalg.solve(A[:, :2], first_map) + rng.normal(0.0, warp_noise, (2, 2))).reshape(4))
    out = dict(plane=np.array(plane[:M], np.int32), x=np.array(x[:M], np.int32), y=np.array(y[:M], np.int32),
               reference=np.array(reference[:M], np.int32), warp0=np.array(warp0[:M], F).reshape(-1, 4))
    if permute:
        order = rng.permutation(M)                          # new position k holds old observation order[k]
        where = np.empty(M, dtype=np.int64)
        where[order] = np.arange(M)
        ref = out["reference"][order]
        out = {k: v[order] for k, v in out.items()}
        out["reference"] = np.where(ref >= 0, where[np.maximum(ref, 0)], -1).astype(np.int32)
    return out


def status_observations():
    """A hand-made list that meets every status: each special observation stands between two good ones."""
    _, rows, planes = collection()
    P = {slot: plane_index(rows, *slot) for slot in _SLOTS}
    good = observations(4, seed=5)                          # one track: a reference and three observations of it
    entries = []                                            # (plane, x, y, reference or a name, warp0)

    def add(plane, x, y, reference, warp=(1.0, 0.0, 0.0, 1.0)):
        entries.append((plane, x, y, reference, tuple(warp)))
        return len(entries) - 1

    def good_pair():
        """A reference and one observation of it."""
        at = len(entries)
        add(good["plane"][0], good["x"][0], good["y"][0], -1)
        add(good["plane"][1], good["x"][1], good["y"][1], at, good["warp0"][1])
        return at

    g0 = good_pair()
    add(good["plane"][2], good["x"][2], good["y"][2], len(entries))            # REFERENCE: names itself
    add(good["plane"][2], good["x"][2], good["y"][2], g0 + 1, np.linalg.solve(      # a reference that is itself a non-reference:
        good["warp0"][1].reshape(2, 2).T, good["warp0"][2].reshape(2, 2).T).T.reshape(4))   # warp(ref -> 2) warp(ref -> 1)^-1
    add(good["plane"][3], good["x"][3], good["y"][3], 10**6, good["warp0"][3])    # BAD_INDEX: reference beyond M
    good_pair()
    add(good["plane"][3], good["x"][3], good["y"][3], -2, good["warp0"][3])       # BAD_INDEX: reference below -1
    add(99, good["x"][1], good["y"][1], g0, good["warp0"][1])                     # BAD_INDEX: own plane beyond the table
    good_pair()
    add(-1, good["x"][1], good["y"][1], g0, good["warp0"][1])                     # BAD_INDEX: own plane negative
    bad_plane_reference = add(77, 5, 5, -1)                                       # REFERENCE (rule 1 comes first) on no plane
    add(good["plane"][1], good["x"][1], good["y"][1], bad_plane_reference)        # BAD_INDEX: the reference's plane
    good_pair()
    add(P[(0, 0)], 48, 20, g0)                                                    # BAD_INDEX: x == W
    add(P[(0, 0)], 20, -1, g0)                                                    # BAD_INDEX: y < 0
    outside_reference = add(P[(1, 0)], 75, 10, -1)                                # REFERENCE with a pixel outside its plane
    add(good["plane"][1], good["x"][1], good["y"][1], outside_reference)          # BAD_INDEX: the reference's pixel
    good_pair()
    border_reference = add(P[(2, 0)], 60, 1, -1)                                  # a reference whose window leaves the plane
    add(good["plane"][1], good["x"][1], good["y"][1], border_reference)           # OUTSIDE: the template
    add(P[(0, 0)], 2, 24, g0)                                                     # OUTSIDE: a warped sample
    add(P[(0, 0)], 24, 24, g0, (3.0, 0.0, 0.0, 3.0))                              # OUTSIDE: the warp leaves a 48 x 48 plane at radius >= 6
    good_pair()
    flat = add(P[(2, 0)], FLAT_BLOCK[0] + 10, FLAT_BLOCK[1] + 10, -1)             # a reference on the constant block
    add(good["plane"][1], good["x"][1], good["y"][1], flat)                       # FLAT: the template
    add(P[(2, 0)], FLAT_BLOCK[0] + 10, FLAT_BLOCK[1] + 10, g0)                    # FLAT: the samples
    add(P[(2, 0)], 60, 50, g0, (0.0, 0.0, 0.0, 0.0))                              # FLAT: a warp that samples one point
    add(P[(2, 0)], CHECKER_BLOCK[0] + 10, CHECKER_BLOCK[1] + 10, g0)              # SINGULAR: every central difference is 0
    good_pair()
    add(P[(2, 0)], 60, 50, g0)                                                    # LOW_CORRELATION (or DIVERGED): another point
    add(P[(1, 0)], 30, 30, g0, (np.nan, 0.0, 0.0, 1.0))                           # OUTSIDE: a NaN warp places no sample
    add(good["plane"][1], good["x"][1] + 2, good["y"][1] - 1, g0, good["warp0"][1])   # a start 2.2 pixels off
    good_pair()
    columns = list(zip(*entries))
    return dict(plane=np.array(columns[0], np.int32), x=np.array(columns[1], np.int32), y=np.array(columns[2], np.int32),
                reference=np.array(columns[3], np.int64).astype(np.int32), warp0=np.array(columns[4], F).reshape(-1, 4))


OPTIONS = dict(radius=7, max_iterations=10, min_step=1e-3, max_shift=3.0, min_correlation=0.8)


def _case(obs, **options):
    return obs, {**OPTIONS, **options}


# name -> (observation list, options); tests/test_gpu_track_refine.py compares every one with the definition byte for byte
@functools.lru_cache(maxsize=None)
def device_cases():
    cases = {}
    for M in (1, 2, 4, 5, 9, 260):
        cases[f"M{M}"] = _case(observations(M))
    cases["M260_permuted"] = _case(observations(260, seed=2, permute=True))
    for radius in (2, 3, 5):
        cases[f"radius{radius}"] = _case(observations(37, seed=3), radius=radius)
    for steps in (1, 3):
        cases[f"iterations{steps}"] = _case(observations(37, seed=4), max_iterations=steps)
    for radius in (3, 7):
        cases[f"statuses_radius{radius}"] = _case(status_observations(), radius=radius)
    cases["diverged"] = _case(observations(37, seed=6, warp_noise=0.0), max_shift=0.1)
    cases["nothing_accepted"] = _case(observations(37, seed=6), min_correlation=1.01)
    cases["far_start"] = _case(observations(37, seed=7, warp_noise=0.15))
    return cases


@functools.lru_cache(maxsize=None)
def expected(name):
    """The definition's result of a device case, computed once."""
    obs, options = device_cases()[name]
    return tro.refine(collection()[2], obs["plane"], obs["x"], obs["y"], obs["reference"], obs["warp0"], **options)


# ---- the stream case ---------------------------------------------------------------------------------------------------------------
STREAM_M = 260


def stream_scene(seed):
    """(level-0 pool bytes, observation arrays) of one scene of the stream case: the collection in another phase, the same list."""
    images, rows, _ = collection(seed)
    return np.concatenate([image.reshape(-1) for image in images]), observations(STREAM_M, seed=8)


@stream_cases.case(["sfm_build_pyramid", "sfm_refine_observations"], [])
def refine_observations(dev):
    """The pyramid of the device collection and the refinement of 260 observations on it, two scenes of equal shapes whose
    textures differ: both C entry points on the test's buffers, sharing one workspace.  There is no torch op."""
    import torch

    from structure_from_motion_amd import device
    from structure_from_motion_amd.feature_matching import keypoints as kp

    i = stream_cases.Inst(dev)
    # three spare streams of torch's pool beside this case: four in all, so that every later side stream of
    # tests/test_gpu_streams.py keeps its hardware queue (the comment in tests/register_views_cases.py)
    i.keep_alignment = [torch.cuda.Stream() for _ in range(3)]
    layout = kp.plan(SHAPES, 1, LEVELS)
    (head_a, obs), (head_b, _) = stream_scene(0), stream_scene(1)
    assert not np.array_equal(head_a, head_b)

    def whole(head):
        pool = np.zeros(layout.pool_bytes, dtype=np.uint8)
        pool[:head.size] = head
        return pool
    pool = i.inp(whole(head_a), whole(head_b))
    i.watch.append(("pool", pool))                       # an input the call also writes: the planes above level 0
    M = STREAM_M
    plane, x, y, reference = (i.same(obs[k], torch.int32) for k in ("plane", "x", "y", "reference"))
    warp0 = i.same(obs["warp0"])
    xy, warp = i.out("xy", (M, 2), torch.float64), i.out("warp", (M, 4), torch.float64)
    correlation = i.out("correlation", (M,), torch.float64)
    iterations, status = i.out("iterations", (M,), torch.int32), i.out("status", (M,), torch.int32)
    i.constant |= {"status"}                              # most observations converge in both scenes
    lib = stream_cases._lib()
    ws = i.work(max(lib.sfm_build_pyramid_workspace_bytes(len(layout.rows)),
                    lib.sfm_refine_observations_workspace_bytes(len(layout.rows))))
    table = device.keypoint_plane_table(layout.rows)
    i.keep = table
    n_planes, n_images = len(layout.rows), len(SHAPES)

    def call():
        st = stream_cases._st()
        stream_cases._check(lib.sfm_build_pyramid(table, n_planes, n_images, pool.data_ptr(), pool.numel(), ws.data_ptr(), ws.numel(),
                                                  st), "sfm_build_pyramid")
        stream_cases._check(lib.sfm_refine_observations(
            table, n_planes, n_images, pool.data_ptr(), pool.numel(), M, plane.data_ptr(), x.data_ptr(), y.data_ptr(),
            reference.data_ptr(), warp0.data_ptr(), 7, 10, 1e-3, 3.0, 0.8, xy.data_ptr(), warp.data_ptr(), correlation.data_ptr(),
            iterations.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), st), "sfm_refine_observations")
    i.call = call
    return i
