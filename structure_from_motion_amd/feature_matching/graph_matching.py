"""Descriptor matching of every image pair of a collection in one ragged device call: from the BRIEF
descriptors of N images to the ``pairs`` and ``matches`` that ``verify_pairs``, ``build_tracks`` and the averaging solvers
take (csrc/sfm_match_pairs.hip, ``device.match_pairs``).

The validation is the standard one, not ``match_brute_force``'s: a row's nearest column within ``max_distance``, Lowe's ratio
against the true runner-up, and a mutual-nearest-neighbour cross-check that asks the ratio of both ends.  The definition is
``tests/graph_matching_oracle.py``; the device result is bit-identical to it.  There is no host fallback.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Sequence

import numpy as np
import numpy.typing as npt

from .brief import DESCRIPTOR_BYTES

MAX_PAIRS_PER_CALL = 65535                # the grid's y extent: one sfm_match_pairs call takes no more
MAX_COLUMN_SLOTS_PER_CALL = 2**27         # pairs x largest image of a call: 1 GiB of column summaries at most
_INT32 = 2**31


class PairMatches(NamedTuple):
    pairs: npt.NDArray                    # (Q, 2) image indices, as given
    matches: List[npt.NDArray]            # per pair (n_q, 2) int64 (a_index, b_index) in ascending a_index
    distances: List[npt.NDArray]          # per pair (n_q,) int32 Hamming distances of those matches


def all_pairs(num_images: int) -> npt.NDArray:
    """Every pair (i, j) with i < j of ``range(num_images)``, in lexicographic order: int64 (Q, 2)."""
    if isinstance(num_images, bool) or not isinstance(num_images, (int, np.integer)) or num_images < 0:
        raise ValueError(f"num_images must be a non-negative integer, got {num_images!r}")
    i, j = np.triu_indices(int(num_images), 1)
    return np.column_stack([i, j]).astype(np.int64).reshape(-1, 2)


def _image_descriptors(value, i: int):
    """``BriefDescriptors`` or (bits, valid) -> ((n, 32) uint8, (n,) uint8 of 0 / 1)."""
    bits, valid = (value.bits, value.valid) if hasattr(value, "bits") and hasattr(value, "valid") else (None, None)
    if bits is None:
        if not isinstance(value, (tuple, list)) or len(value) != 2:
            raise TypeError(f"descriptors[{i}] must be BriefDescriptors or a (bits, valid) pair")
        bits, valid = value
    bits, valid = np.asarray(bits), np.asarray(valid)
    if bits.dtype != np.uint8:
        raise TypeError(f"descriptors[{i}]: bits must be uint8, got {bits.dtype}")
    if valid.dtype != np.bool_ and not np.issubdtype(valid.dtype, np.integer):
        raise TypeError(f"descriptors[{i}]: valid must be boolean or integer flags, got {valid.dtype}")
    if bits.size == 0 and valid.size == 0:
        return np.zeros((0, DESCRIPTOR_BYTES), np.uint8), np.zeros(0, np.uint8)
    if bits.ndim != 2 or bits.shape[1] != DESCRIPTOR_BYTES or valid.shape != (bits.shape[0],):
        raise ValueError(f"descriptors[{i}] must be (n, {DESCRIPTOR_BYTES}) bits with (n,) validity flags, got {bits.shape} "
                         f"and {valid.shape}")
    return np.ascontiguousarray(bits), np.ascontiguousarray(valid != 0, dtype=np.uint8)


def _checked_arguments(descriptors: Sequence, pairs, max_distance, ratio, cross_check, max_pairs_per_call):
    """Every check of ``match_image_pairs``, in ``view_graph._checked_graph``'s style -> (descriptors per image, (Q, 2) pairs,
    max_distance, ratio or None, cross_check, max_pairs_per_call)."""
    images = [_image_descriptors(d, i) for i, d in enumerate(descriptors)]
    pair_arr = np.asarray(pairs)
    if pair_arr.size == 0:
        pair_arr = np.zeros((0, 2), dtype=np.int64)
    if pair_arr.ndim != 2 or pair_arr.shape[1] != 2:
        raise ValueError(f"pairs must have shape (Q, 2), got {pair_arr.shape}")
    if not np.issubdtype(pair_arr.dtype, np.integer):
        raise ValueError(f"pairs must hold integers, got {pair_arr.dtype}")
    Q = pair_arr.shape[0]
    if Q and (pair_arr.min() < 0 or pair_arr.max() >= len(images)):
        raise ValueError(f"pairs must index images 0 .. {len(images) - 1}")
    if Q and np.any(pair_arr[:, 0] == pair_arr[:, 1]):
        raise ValueError("a pair must join two different images")
    if isinstance(max_distance, bool) or not isinstance(max_distance, (int, np.integer)) or not 0 <= max_distance <= 256:
        raise ValueError(f"max_distance must be an integer in 0 .. 256, got {max_distance!r}")
    if ratio is not None:
        if isinstance(ratio, bool) or not isinstance(ratio, (int, float, np.integer, np.floating)):
            raise TypeError(f"ratio must be a number or None, got {ratio!r}")
        ratio = float(ratio)
        if not (math.isfinite(ratio) and ratio > 0.0):
            raise ValueError(f"ratio must be finite and positive, or None, got {ratio!r}")
    if not isinstance(cross_check, (bool, np.bool_)):
        raise TypeError(f"cross_check must be a bool, got {cross_check!r}")
    if (isinstance(max_pairs_per_call, bool) or not isinstance(max_pairs_per_call, (int, np.integer))
            or not 1 <= max_pairs_per_call <= MAX_PAIRS_PER_CALL):
        raise ValueError(f"max_pairs_per_call must be an integer in 1 .. {MAX_PAIRS_PER_CALL}, got {max_pairs_per_call!r}")
    sizes = np.array([len(v) for _, v in images], dtype=np.int64)
    if sizes.sum() >= _INT32:
        raise ValueError("descriptors must number fewer than 2^31")
    if Q and sizes[pair_arr[:, 0]].sum() >= _INT32:
        raise ValueError("the first images of the pairs must hold fewer than 2^31 descriptors in total")
    return images, pair_arr.astype(np.int64), int(max_distance), ratio, bool(cross_check), int(max_pairs_per_call)


def call_bounds(sizes, pair_arr, max_pairs_per_call: int) -> List[tuple]:
    """``[(q0, q1), ...]``: the pairs of each device call — at most ``max_pairs_per_call`` and, beyond the first pair, at most
    ``MAX_COLUMN_SLOTS_PER_CALL`` column summaries (pairs x the largest image any pair of the call names)."""
    bounds, q0, largest = [], 0, 0
    for q, (i, j) in enumerate(pair_arr.tolist()):
        grown = max(largest, int(sizes[i]), int(sizes[j]))
        if q > q0 and (q - q0 >= max_pairs_per_call or (q - q0 + 1) * grown > MAX_COLUMN_SLOTS_PER_CALL):
            bounds.append((q0, q))
            q0, grown = q, max(int(sizes[i]), int(sizes[j]))
        largest = grown
    if len(pair_arr) > q0:
        bounds.append((q0, len(pair_arr)))
    return bounds


def match_image_pairs(descriptors: Sequence, pairs, *, max_distance: int = 64, ratio=0.8, cross_check: bool = True,
                      max_pairs_per_call: int = MAX_PAIRS_PER_CALL) -> PairMatches:
    """Match the descriptors of every image pair of ``pairs`` on the GPU (``sfm_match_pairs``).

    ``descriptors[i]`` is image i's ``BriefDescriptors`` (``compute_brief``) or a ``(bits (n, 32) uint8, valid (n,))`` pair;
    ``pairs`` is ``(Q, 2)`` image indices, two different images per pair (``all_pairs`` lists every one).  For pair (i, j) a
    feature a of image i keeps its nearest feature b of image j (Hamming distance, the smallest b on a tie) iff the distance
    is at most ``max_distance``, it is at most ``ratio`` times the distance to a's runner-up in image j (``ratio=None``: no
    ratio test; a tie for the best fails every ratio below 1) and, with ``cross_check``, a is also b's nearest feature of
    image i and passes the ratio test against b's runner-up there.  Invalid descriptors never match.  With ``cross_check``
    the matches of (j, i) are exactly those of (i, j) transposed and no feature appears twice in a list.

    All descriptors go to the device in one upload and all rows come back in one read; the host only compacts them.  The
    pairs are split into device calls of at most ``max_pairs_per_call``, which does not change the result.  ``matches`` is
    what ``verify_pairs`` and ``build_tracks`` take.  Every argument is checked before any device work (``ValueError`` /
    ``TypeError``); no pairs, or no features in any first image, need no GPU."""
    images, pair_arr, max_distance, ratio, cross_check, per_call = _checked_arguments(
        descriptors, pairs, max_distance, ratio, cross_check, max_pairs_per_call)
    Q = len(pair_arr)
    sizes = np.array([len(v) for _, v in images], dtype=np.int64)
    row_offset = np.zeros(Q + 1, dtype=np.int64)
    row_offset[1:] = np.cumsum(sizes[pair_arr[:, 0]])
    rows = int(row_offset[-1])
    if rows == 0:
        return PairMatches(pair_arr, [np.zeros((0, 2), np.int64) for _ in range(Q)], [np.zeros(0, np.int32) for _ in range(Q)])
    import torch

    from .. import device

    dev = device.require_gpu()
    I, F = len(images), int(sizes.sum())
    chunks = call_bounds(sizes, pair_arr, per_call)
    # one upload: descriptors | flags | per call its row offsets from 0 (int64) | image offsets | pair images (int32)
    call_rows = [row_offset[q0:q1 + 1] - row_offset[q0] for q0, q1 in chunks]
    image_offset = np.zeros(I + 1, dtype=np.int32)
    image_offset[1:] = np.cumsum(sizes)
    at_ok = F * DESCRIPTOR_BYTES
    at_rows = (at_ok + F + 7) // 8 * 8
    at_images = at_rows + 8 * sum(len(r) for r in call_rows)
    at_pairs = at_images + 4 * (I + 1)
    host = np.zeros(at_pairs + 8 * Q, dtype=np.uint8)
    host[:at_ok] = np.concatenate([b for b, _ in images]).reshape(-1)
    host[at_ok:at_ok + F] = np.concatenate([v for _, v in images])
    host[at_rows:at_images] = np.concatenate(call_rows).view(np.uint8)
    host[at_images:at_pairs] = image_offset.view(np.uint8)
    host[at_pairs:] = np.ascontiguousarray(pair_arr, dtype=np.int32).reshape(-1).view(np.uint8)
    buf = torch.as_tensor(host).to(dev)
    desc, ok = buf[:at_ok], buf[at_ok:at_ok + F]
    rows_dev = buf[at_rows:at_images].view(torch.int64)
    image_offset_dev = buf[at_images:at_pairs].view(torch.int32)
    pair_images_dev = buf[at_pairs:].view(torch.int32).view(Q, 2)
    out = torch.empty((2 * rows + Q,), dtype=torch.int32, device=dev)   # partner | distance | pair status: one read
    partner, distance, status = out[:rows], out[rows:2 * rows], out[2 * rows:]
    workspace, at = None, 0
    for (q0, q1), r in zip(chunks, call_rows):
        lo, hi = int(row_offset[q0]), int(row_offset[q1])
        largest = int(sizes[pair_arr[q0:q1]].max())
        workspace = device.match_pairs(I, F, image_offset_dev, desc, ok, pair_images_dev[q0:q1], rows_dev[at:at + len(r)],
                                       hi - lo, largest, max_distance, ratio, cross_check, partner[lo:hi], distance[lo:hi],
                                       status[q0:q1], workspace)
        at += len(r)
    result = out.cpu().numpy()
    if np.any(result[2 * rows:] != 0):
        raise RuntimeError("match_image_pairs: the device refused a pair the host had checked (sfm_match_pairs pair_status)")
    partner_host, distance_host = result[:rows], result[rows:2 * rows]
    kept = np.nonzero(partner_host >= 0)[0]
    owner = np.searchsorted(row_offset, kept, side="right") - 1
    table = np.column_stack([kept - row_offset[owner], partner_host[kept].astype(np.int64)]).astype(np.int64).reshape(-1, 2)
    cuts = np.searchsorted(kept, row_offset[1:-1], side="left")
    return PairMatches(pair_arr, np.split(table, cuts), np.split(distance_host[kept], cuts))
