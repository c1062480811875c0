"""GPU tests of the graph matcher (csrc/sfm_match_pairs.hip): partner and distance byte for byte against the NumPy definition
(tests/graph_matching_oracle.py) on the smallest collection that crosses every boundary of the kernels, against the existing
Hamming summary, through the C ABI with pairs the device must refuse, and through the app."""
import functools

import numpy as np
import pytest

import graph_matching_oracle as gmo

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _gpu(native_lib):
    from structure_from_motion_amd import device

    device.require_gpu()


from structure_from_motion_amd import device  # noqa: E402
from structure_from_motion_amd.feature_matching import _device_match  # noqa: E402
from structure_from_motion_amd.feature_matching.graph_matching import all_pairs, match_image_pairs  # noqa: E402

# no features, one, two, a row block less one / exactly / plus one (256), an LDS tile plus one (512), two tiles and five row blocks
SIZES = (0, 1, 2, 255, 256, 257, 513, 1030)
ALL_INVALID, ONE_VALID = 3, 5                       # image 3 has no valid descriptor; image 5 exactly one, in its last row block
PAIRS = [(i, j) for i in range(len(SIZES)) for j in range(len(SIZES)) if i != j] + [(7, 6)]   # 56 ordered pairs, one repeated
FAMILIES = ("random", "ties", "noisy")
OPTIONS = [(ratio, max_distance, cross_check) for ratio in (None, 0.8, 1.0) for max_distance in (0, 64, 256)
           for cross_check in (False, True)]


@functools.lru_cache(maxsize=None)
def collection(family):
    """(descriptors per image, the oracle's summaries of PAIRS): computed once, shared by every test, never changed."""
    rng = np.random.default_rng(FAMILIES.index(family) + 40)
    pool = rng.integers(0, 256, (400, 32), dtype=np.uint8)
    three = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    images = []
    for k, n in enumerate(SIZES):
        if family == "random":
            bits = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        elif family == "ties":
            bits = three[rng.integers(0, 3, n)]      # three values: ties for the best and the runner-up everywhere
        else:
            flips = np.zeros((n, 256), dtype=np.uint8)
            for row, count in zip(flips, rng.integers(0, 41, n)):   # a pool descriptor with 0 .. 40 flipped bits: real matches
                row[rng.choice(256, count, replace=False)] = 1
            bits = pool[rng.integers(0, len(pool), n)] ^ np.packbits(flips, axis=1, bitorder="little")
        valid = rng.random(n) < 0.9                  # scattered invalid features
        if k == ALL_INVALID:
            valid[:] = False
        if k == ONE_VALID:
            valid[:] = False
            valid[n - 1] = True
        bits.setflags(write=False)
        valid.setflags(write=False)
        images.append((bits, valid))
    return images, gmo.GraphSummaries(images, PAIRS)


class Resident:
    """One collection on the device, in sfm_match_pairs's layout, for calls through the C ABI."""

    def __init__(self, images):
        self.sizes = np.array([len(v) for _, v in images], dtype=np.int64)
        self.I, self.F = len(images), int(self.sizes.sum())
        offset = np.zeros(self.I + 1, dtype=np.int32)
        offset[1:] = np.cumsum(self.sizes)
        self.image_offset = device.to_device(offset, torch.int32)
        self.desc = device.to_device(np.concatenate([b for b, _ in images]), torch.uint8)
        self.ok = device.to_device(np.concatenate([v for _, v in images]).astype(np.uint8), torch.uint8)

    def rows(self, pairs, ratio, max_distance, cross_check, row_offset=None, max_n=None):
        """(partner, distance, pair_status) of one call; ``row_offset`` / ``max_n`` default to the honest ones."""
        pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        if row_offset is None:
            row_offset = np.zeros(len(pairs) + 1, dtype=np.int64)
            row_offset[1:] = np.cumsum(self.sizes[pairs[:, 0]])
        rows = int(row_offset[-1])
        out = torch.full((2 * rows + len(pairs),), 77, dtype=torch.int32, device=self.desc.device)   # 77: never a result
        device.match_pairs(self.I, self.F, self.image_offset, self.desc, self.ok, device.to_device(pairs, torch.int32),
                           device.to_device(row_offset, torch.int64), rows, int(self.sizes.max()) if max_n is None else max_n,
                           max_distance, ratio, cross_check, out[:rows], out[rows:2 * rows], out[2 * rows:])
        host = out.cpu().numpy()
        return host[:rows], host[rows:2 * rows], host[2 * rows:]


@pytest.mark.parametrize("family", FAMILIES)
def test_rows_byte_equal_the_definition(family):
    images, summaries = collection(family)
    resident = Resident(images)
    for ratio, max_distance, cross_check in OPTIONS:
        want_partner, want_distance, _ = summaries.rows(max_distance, ratio, cross_check)
        partner, distance, status = resident.rows(PAIRS, ratio, max_distance, cross_check)
        assert partner.dtype == np.int32 and distance.dtype == np.int32
        assert not status.any()
        assert partner.tobytes() == want_partner.tobytes(), (ratio, max_distance, cross_check)
        assert distance.tobytes() == want_distance.tobytes(), (ratio, max_distance, cross_check)
    # the tests must have had something to decide
    assert np.count_nonzero(summaries.rows(256, None, False)[0] >= 0) > 1000
    assert family != "noisy" or np.count_nonzero(summaries.rows(64, 0.8, True)[0] >= 0) > 100
    again = resident.rows(PAIRS, 0.8, 64, True)
    once = resident.rows(PAIRS, 0.8, 64, True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, once))


@pytest.mark.parametrize("family", FAMILIES)
def test_match_image_pairs_lists_and_call_splitting(family):
    images, summaries = collection(family)
    want_matches, want_distances = summaries.matches(64, 0.8, True)
    got = match_image_pairs(images, PAIRS)
    assert got.pairs.dtype == np.int64 and got.pairs.tolist() == [list(p) for p in PAIRS]
    split = match_image_pairs(images, PAIRS, max_pairs_per_call=3)
    twice = match_image_pairs(images, PAIRS)
    assert len(got.matches) == len(got.distances) == len(PAIRS)
    for q in range(len(PAIRS)):
        assert got.matches[q].dtype == np.int64 and got.matches[q].shape == (len(want_distances[q]), 2)
        assert got.distances[q].dtype == np.int32
        assert np.array_equal(got.matches[q], want_matches[q]) and np.array_equal(got.distances[q], want_distances[q])
        for other in (split, twice):
            assert np.array_equal(other.matches[q], got.matches[q]) and np.array_equal(other.distances[q], got.distances[q])
    # other options through the public call, the ratio test off included
    loose = match_image_pairs(images, PAIRS, max_distance=256, ratio=None, cross_check=False, max_pairs_per_call=20)
    want_matches, want_distances = summaries.matches(256, None, False)
    for q in range(len(PAIRS)):
        assert np.array_equal(loose.matches[q], want_matches[q]) and np.array_equal(loose.distances[q], want_distances[q])


@pytest.mark.parametrize("family", FAMILIES)
def test_reversed_pairs_give_the_transposed_sets(family):
    images, _ = collection(family)
    forward = all_pairs(len(SIZES))
    a = match_image_pairs(images, forward, ratio=1.0, max_distance=256)
    b = match_image_pairs(images, forward[:, ::-1], ratio=1.0, max_distance=256)
    total = 0
    for m, d, back, back_d in zip(a.matches, a.distances, b.matches, b.distances):
        order = np.argsort(m[:, 1], kind="stable")
        assert np.array_equal(m[order][:, ::-1], back) and np.array_equal(d[order], back_d)
        assert len(np.unique(m[:, 0])) == len(m) and len(np.unique(m[:, 1])) == len(m)
        total += len(m)
    assert total > 0


@pytest.mark.parametrize("family", ("ties", "noisy"))
def test_nearest_agrees_with_the_hamming_summary(family):
    images, _ = collection(family)
    pairs = [(i, j) for i, j in PAIRS[:-1] if SIZES[i] and SIZES[j]]
    got = Resident(images).rows(pairs, None, 256, False)
    offset = np.concatenate([[0], np.cumsum([SIZES[i] for i, _ in pairs])])
    finite = 0
    for q, (i, j) in enumerate(pairs):
        best, arg, _ = _device_match.hamming_summary(*(np.array(x) for x in images[i] + images[j]))   # copies: the shared arrays are read-only
        partner, distance = got[0][offset[q]:offset[q + 1]], got[1][offset[q]:offset[q + 1]]
        there = np.isfinite(best)
        assert np.array_equal(there, partner >= 0)
        assert np.array_equal(partner[there], arg[there]) and np.array_equal(distance[there], best[there].astype(np.int32))
        finite += int(there.sum())
    assert finite > 1000


def _expect(summaries, pairs, bad, spans, ratio, max_distance, cross_check):
    """Rows of a call whose pairs ``bad`` (indices) the device must refuse: -1 over their spans, the oracle's elsewhere."""
    by_pair = {p: gmo.decide(summaries.per_pair[p], max_distance, ratio, cross_check) for p in set(pairs) if p in summaries.per_pair}
    partner, distance = [], []
    for q, p in enumerate(pairs):
        if q in bad:
            partner.append(np.full(spans[q], -1, np.int32))
            distance.append(np.full(spans[q], -1, np.int32))
        else:
            partner.append(by_pair[p][0])
            distance.append(by_pair[p][1])
    return np.concatenate(partner), np.concatenate(distance)


@pytest.mark.parametrize("case", ("image_out_of_range", "same_image", "wrong_span", "understated_max"))
def test_c_abi_refuses_a_pair_and_serves_the_others(case):
    images, summaries = collection("noisy")
    resident = Resident(images)
    pairs = [(7, 6), (4, 7), (6, 5), (2, 7), (7, 4), (1, 6)]
    spans = [SIZES[i] for i, _ in pairs]
    max_n = None
    if case == "image_out_of_range":
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
        want = _expect(summaries, pairs, bad, spans, ratio, max_distance, cross_check)
        partner, distance, status = resident.rows(pairs, ratio, max_distance, cross_check, row_offset, max_n)
        assert status.tolist() == [int(q in bad) for q in range(len(pairs))]
        assert partner.tobytes() == want[0].tobytes() and distance.tobytes() == want[1].tobytes()
        assert ratio is not None or np.count_nonzero(partner >= 0) > 100


def test_app_matches_equal_the_definition():
    from apps import match_image_collection as app

    record, (descriptors, matched, graph, tracks) = app.run(degrees=(0.0, 17.0, 45.0, 90.0), height=240, width=320,
                                                            features=200, extra=60, details=True)
    pairs = all_pairs(4)
    assert np.array_equal(matched.pairs, pairs) and len(record["pairs"]) == 6
    want, _ = gmo.match_graph([(d.bits, d.valid) for d in descriptors], pairs, 64, 0.8, True)
    from structure_from_motion_amd import synthetic

    _, _, ids = synthetic.rotated_texture_views(240, 320, (0.0, 17.0, 45.0, 90.0), 200, 60, 7)
    for q, (i, j) in enumerate(pairs.tolist()):
        assert np.array_equal(matched.matches[q], want[q])
        right = sum(1 for a, b in want[q].tolist() if ids[i][a] >= 0 and ids[i][a] == ids[j][b])
        entry = record["pairs"][q]
        assert entry["images"] == [i, j] and entry["kept"] == len(want[q])
        assert entry["precision"] == right / len(want[q]) and entry["recall"] == right / 200
        assert entry["kind"] == graph.kind[q] == "homography"    # a rotation about the principal point
    print(record)
    assert record["tracks"] == tracks.info.tracks
