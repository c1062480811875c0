"""GPU tests of guided matching (match_pairs_guided_kernel of csrc/sfm_match_pairs.hip): partner, distance and pair_status
byte for byte against the NumPy definition (tests/guided_matching_oracle.py) on the smallest collection that crosses every
boundary of the kernel, the identities, the pairs the device must refuse, the end-to-end chain on repeated structure and the
app."""
import functools

import numpy as np
import pytest

import guided_matching_cases as gc
import guided_matching_oracle as go

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _gpu(native_lib):
    from structure_from_motion_amd import device

    device.require_gpu()


from structure_from_motion_amd import device  # noqa: E402
from structure_from_motion_amd.feature_matching.guided_matching import guided_match_models, guided_match_pairs  # noqa: E402

SIZES, PAIRS = gc.SIZES, gc.PAIRS
K = np.array([[1000.0, 0.0, 320.0], [0.0, 1000.0, 240.0], [0.0, 0.0, 1.0]])


class Resident:
    """One collection on the device, in sfm_match_pairs_guided's layout, for calls through the C ABI."""

    def __init__(self, images):
        self.sizes = np.array([len(im[1]) for im in images], dtype=np.int64)
        self.I, self.F = len(images), int(self.sizes.sum())
        offset = np.zeros(self.I + 1, dtype=np.int32)
        offset[1:] = np.cumsum(self.sizes)
        self.image_offset = device.to_device(offset, torch.int32)
        self.desc = device.to_device(np.concatenate([im[0] for im in images]), torch.uint8)
        self.ok = device.to_device(np.concatenate([im[1] for im in images]).astype(np.uint8), torch.uint8)
        self.xy = device.to_device(np.concatenate([im[2] for im in images]), torch.float64)

    def _arguments(self, pairs, row_offset):
        pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        if row_offset is None:
            row_offset = np.zeros(len(pairs) + 1, dtype=np.int64)
            row_offset[1:] = np.cumsum(self.sizes[pairs[:, 0]])
        rows = int(row_offset[-1])
        out = torch.full((2 * rows + len(pairs),), 77, dtype=torch.int32, device=self.desc.device)   # 77: never a result
        return pairs, row_offset, rows, out

    @staticmethod
    def _host(out, rows):
        host = out.cpu().numpy()
        return host[:rows], host[rows:2 * rows], host[2 * rows:]

    def rows(self, pairs, models, kinds, thresholds, ratio, max_distance, cross_check, row_offset=None, max_n=None):
        """(partner, distance, pair_status) of one guided call; ``row_offset`` / ``max_n`` default to the honest ones."""
        pairs, row_offset, rows, out = self._arguments(pairs, row_offset)
        device.match_pairs_guided(
            self.I, self.F, self.image_offset, self.desc, self.ok, self.xy, device.to_device(pairs, torch.int32),
            device.to_device(row_offset, torch.int64), device.to_device(np.asarray(models, np.float64).reshape(-1, 9), torch.float64),
            device.to_device(np.asarray(kinds, np.int32), torch.int32), device.to_device(np.asarray(thresholds, np.float64), torch.float64),
            rows, int(self.sizes.max()) if max_n is None else max_n, max_distance, ratio, cross_check, out[:rows],
            out[rows:2 * rows], out[2 * rows:])
        return self._host(out, rows)

    def unguided(self, pairs, ratio, max_distance, cross_check):
        pairs, row_offset, rows, out = self._arguments(pairs, None)
        device.match_pairs(self.I, self.F, self.image_offset, self.desc, self.ok, device.to_device(pairs, torch.int32),
                           device.to_device(row_offset, torch.int64), rows, int(self.sizes.max()), max_distance, ratio, cross_check,
                           out[:rows], out[rows:2 * rows], out[2 * rows:])
        return self._host(out, rows)


@pytest.mark.parametrize("family", gc.FAMILIES)
def test_rows_byte_equal_the_definition(family):
    col = gc.collection(family)
    resident = Resident(col.images)
    for ratio, max_distance, cross_check in gc.OPTIONS:
        want_partner, want_distance = col.rows(max_distance, ratio, cross_check)
        partner, distance, status = resident.rows(PAIRS, col.models, col.kinds, col.thresholds, ratio, max_distance, cross_check)
        assert partner.dtype == np.int32 and distance.dtype == np.int32
        assert not status.any()
        assert partner.tobytes() == want_partner.tobytes(), (ratio, max_distance, cross_check)
        assert distance.tobytes() == want_distance.tobytes(), (ratio, max_distance, cross_check)
    # the tests must have had something to decide, and the gate something to remove
    loose = col.rows(256, None, False)[0]
    assert np.count_nonzero(loose >= 0) > 1000
    assert np.count_nonzero(loose != col.unguided.rows(256, None, False)[0]) > 1000
    assert family != "noisy" or np.count_nonzero(col.rows(64, 0.8, True)[0] >= 0) > 100
    again = resident.rows(PAIRS, col.models, col.kinds, col.thresholds, 0.8, 64, True)
    once = resident.rows(PAIRS, col.models, col.kinds, col.thresholds, 0.8, 64, True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, once))


@pytest.mark.parametrize("family", gc.FAMILIES)
def test_identity_homography_with_infinite_threshold_is_the_unguided_call(family):
    col = gc.collection(family)
    resident = Resident(col.images)
    Q = len(PAIRS)
    identity, kinds, thresholds = np.tile(np.eye(3), (Q, 1, 1)), np.full(Q, go.KIND_HOMOGRAPHY), np.full(Q, np.inf)
    for ratio, max_distance, cross_check in ((0.8, 64, True), (None, 256, False), (1.0, 256, True)):
        guided = resident.rows(PAIRS, identity, kinds, thresholds, ratio, max_distance, cross_check)
        plain = resident.unguided(PAIRS, ratio, max_distance, cross_check)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(guided, plain))
        assert ratio is not None or np.count_nonzero(plain[0] >= 0) > 1000   # every valid row with a valid column


@pytest.mark.parametrize("family", gc.FAMILIES)
def test_guided_match_models_lists_and_call_splitting(family):
    col = gc.collection(family)
    descriptors = [im[:2] for im in col.images]
    pixels = [im[2] * np.array([K[0, 0], K[1, 1]]) + np.array([K[0, 2], K[1, 2]]) for im in col.images]
    # the coordinates the call derives from the pixels are the definition's inputs here
    from structure_from_motion_amd.feature_matching.guided_matching import normalized_coordinates

    images = [(b, v, normalized_coordinates(K, p)) for (b, v), p in zip(descriptors, pixels)]
    names = [("none", "essential", "homography")[k] for k in col.kinds]
    want_matches, want_distances = go.match_graph(images, PAIRS, col.models, col.kinds, col.thresholds)
    got = guided_match_models(descriptors, pixels, K, PAIRS, col.models, names, col.thresholds)
    split = guided_match_models(descriptors, pixels, K, PAIRS, col.models, col.kinds, col.thresholds, max_pairs_per_call=3)
    twice = guided_match_models(descriptors, pixels, K, PAIRS, col.models, names, col.thresholds)
    assert got.pairs.dtype == np.int64 and got.pairs.tolist() == [list(p) for p in PAIRS]
    assert len(got.matches) == len(got.distances) == len(PAIRS)
    for q in range(len(PAIRS)):
        assert got.matches[q].dtype == np.int64 and got.matches[q].shape == (len(want_distances[q]), 2)
        assert got.distances[q].dtype == np.int32
        assert np.array_equal(got.matches[q], want_matches[q]) and np.array_equal(got.distances[q], want_distances[q])
        for other in (split, twice):
            assert np.array_equal(other.matches[q], got.matches[q]) and np.array_equal(other.distances[q], got.distances[q])
        assert len(np.unique(got.matches[q][:, 0])) == len(got.matches[q]) == len(np.unique(got.matches[q][:, 1]))
    assert sum(len(m) for m in got.matches) > (100 if family == "noisy" else -1)
    # a scalar threshold and other options through the public call
    loose = guided_match_models(descriptors, pixels, K, PAIRS, col.models, names, 1e-3, max_distance=256, ratio=None,
                                cross_check=False, max_pairs_per_call=20)
    want_matches, want_distances = go.match_graph(images, PAIRS, col.models, col.kinds, [1e-3] * len(PAIRS), 256, None, False)
    for q in range(len(PAIRS)):
        assert np.array_equal(loose.matches[q], want_matches[q]) and np.array_equal(loose.distances[q], want_distances[q])
    assert sum(len(m) for m in loose.matches) > 1000


REFUSAL_PAIRS = ((7, 6), (4, 7), (6, 5), (2, 7), (7, 4), (1, 6))


@functools.lru_cache(maxsize=None)
def refusal_call():
    """Six pairs of the noisy collection, essential and homography in turn with bands that admit about half: (models, kinds,
    thresholds, the oracle's summaries per pair)."""
    col = gc.collection("noisy")
    kinds = np.array([gc.KIND_CYCLE[k % 2] for k in range(len(REFUSAL_PAIRS))], dtype=np.int32)
    models = np.array([gc.motion_model(("bench", "plane_bench")[k % 2], kinds[k]) for k in range(len(REFUSAL_PAIRS))])
    thresholds = np.array([gc.band_threshold(go.errors(models[k], kinds[k], col.images[i][2], col.images[j][2]), "wide")
                           for k, (i, j) in enumerate(REFUSAL_PAIRS)])
    summaries = [go.pair_summaries(col.images[i], col.images[j], models[k], kinds[k], thresholds[k])
                 for k, (i, j) in enumerate(REFUSAL_PAIRS)]
    return models, kinds, thresholds, summaries


@pytest.mark.parametrize("case", ("unknown_kind", "image_out_of_range", "same_image", "wrong_span", "understated_max"))
def test_c_abi_refuses_a_pair_and_serves_the_others(case):
    import graph_matching_oracle as gmo

    resident = Resident(gc.collection("noisy").images)
    models, kinds, thresholds, summaries = refusal_call()
    pairs, kinds = list(REFUSAL_PAIRS), kinds.copy()
    spans = [SIZES[i] for i, _ in pairs]
    max_n = None
    if case == "unknown_kind":
        kinds[0], kinds[2], kinds[5] = 3, -1, 2**31 - 1
        bad = {0, 2, 5}
    elif case == "image_out_of_range":
        pairs[1], pairs[3], pairs[5] = (4, 8), (-1, 7), (2**31 - 1, 6)   # the second image, the first image, far out
        bad = {1, 3, 5}
        spans[3], spans[5] = 300, 0                # whatever span such a pair is given is -1
    elif case == "same_image":
        pairs[2] = (6, 6)
        bad = {2}
    elif case == "wrong_span":
        spans[0], spans[4] = 1029, 1031            # one row short, one row long
        bad = {0, 4}
    else:
        max_n = 1029                               # image 7 has 1030 features: every pair that names it is refused
        bad = {0, 1, 3, 4}
    row_offset = np.concatenate([[0], np.cumsum(spans)]).astype(np.int64)
    for ratio, max_distance, cross_check in ((0.8, 64, True), (None, 256, False)):
        want_partner, want_distance = [], []
        for k in range(len(pairs)):
            p, d = (np.full(spans[k], -1, np.int32),) * 2 if k in bad else gmo.decide(summaries[k], max_distance, ratio, cross_check)
            want_partner.append(p), want_distance.append(d)
        partner, distance, status = resident.rows(pairs, models, kinds, thresholds, ratio, max_distance, cross_check, row_offset,
                                                  max_n)
        assert status.tolist() == [int(k in bad) for k in range(len(pairs))]
        assert partner.tobytes() == np.concatenate(want_partner).tobytes()
        assert distance.tobytes() == np.concatenate(want_distance).tobytes()
        assert ratio is not None or np.count_nonzero(partner >= 0) > 100


def test_stream_case_is_registered_and_runs():
    """The protocol itself runs in tests/test_gpu_streams.py; here the case's two scenes must give different, non-trivial
    results on the default stream."""
    import stream_cases

    inst = stream_cases.CASES["match_pairs_guided"].build(device.require_gpu())
    results = []
    for scene in "AB":
        inst.load(scene)
        inst.call()
        torch.cuda.synchronize()
        results.append([o.cpu().numpy().copy() for o in inst.Out])
    assert not results[0][2].any() and not results[1][2].any()
    assert np.count_nonzero(results[0][0] >= 0) > 100 and results[0][0].tobytes() != results[1][0].tobytes()


CHAIN_SEED = 21        # the scene
VERIFY_SEED = 5        # verify_pairs's sampling seed


def test_end_to_end_gain_on_repeated_structure():
    """First pass, verification with refined poses, guided pass with those poses; the gain in right matches over the twelve
    pairs must reach half of the gain with the true essential matrices (G_true, from the NumPy definition)."""
    from structure_from_motion_amd.epipolar.view_graph import verify_pairs
    from structure_from_motion_amd.feature_matching.graph_matching import match_image_pairs
    from structure_from_motion_amd.multiview.tracks import build_tracks

    chain = gc.repeated_chain(CHAIN_SEED)
    sc, pairs = chain["scene"], chain["pairs"]
    first = match_image_pairs(sc["descriptors"], pairs)
    for q in range(len(pairs)):
        assert np.array_equal(first.matches[q], chain["first"][q])
    # the gate of the app: without one the lowest RMS wins on a handful of items and the pair keeps a model of six inliers
    graph = verify_pairs(sc["K"], sc["pixels"], pairs, first.matches, gc.THR, min_extra_fraction=0.4, max_iterations=256,
                         seed=VERIFY_SEED, relative_pose=True, refine_pose_rounds=2)
    assert "none" not in graph.kind, graph.kind
    guided = guided_match_pairs(sc["descriptors"], sc["pixels"], sc["K"], graph, gc.THR, use_pose=True)
    g_true = sum(r[4] - r[2] for r in chain["rows"])
    gains = []
    for q, (i, j) in enumerate(pairs.tolist()):
        right = gc.right_matches(guided.matches[q], sc["ids"][i], sc["ids"][j])
        gains.append(right - chain["rows"][q][2])
        print(f"pair {(i, j)} {graph.kind[q]} {graph.pose.status[q]}: common {chain['rows'][q][0]}, first pass "
              f"{chain['rows'][q][2]} right of {chain['rows'][q][1]}, guided {right} right of {len(guided.matches[q])}, with the "
              f"true E {chain['rows'][q][4]} right of {chain['rows'][q][3]}")
    print(f"device gain {sum(gains)}, G_true {g_true}")
    assert g_true > 1000
    assert sum(gains) >= 0.5 * g_true
    # its lists are what the later stages take
    again = verify_pairs(sc["K"], sc["pixels"], pairs, guided.matches, gc.THR, max_iterations=64, seed=VERIFY_SEED)
    tracks = build_tracks(sc["pixels"], pairs, again.inlier_matches)
    assert tracks.info.tracks > 0


def test_app_repeated_guided_lists_equal_the_definition():
    from apps import match_image_collection as app

    record, details = app.run(scene="repeated", guided=True, views=3, features=200, unique=120, groups=16, extra=40, seed=21,
                              inlier_threshold=gc.THR, iterations=128, details=True)
    descriptors, matched, _, tracks, guided, features, K, graph = details
    from structure_from_motion_amd.feature_matching.guided_matching import graph_models, normalized_coordinates

    images = [(d[0], d[1], normalized_coordinates(K, f)) for d, f in zip(descriptors, features)]
    models, kinds = graph_models(graph, use_pose=True)
    want, _ = go.match_graph(images, graph.pairs, models, [go.KIND_CODES[k] for k in kinds], [gc.THR] * len(kinds))
    assert len(record["pairs"]) == len(want) == 3
    for q in range(len(want)):
        assert np.array_equal(guided.matches[q], want[q])
        assert record["pairs"][q]["guided"]["kept"] == len(want[q])
    assert sum(len(m) for m in want) > sum(len(m) for m in matched.matches)
    print(record)
