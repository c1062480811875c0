"""Timing of the ragged similarity alignment (``sfm_align_models``) next to the loop of single-pair calls it
replaces, for profiles/align_models/README.md: 64 pairs of 200 to 5 000 items each, 1 000 hypotheses per pair, two refit
rounds.  One JSON line with

* ``ragged_device_ms``: ``AlignModelsWorkspace.run`` on device-resident inputs, HIP events around the call;
* ``single_device_ms``: the sum over the pairs of ``SimilarityWorkspace(1, n_q, h).run`` + ``.refine`` on the same items, HIP
  events around each pair's two calls (the workspaces allocated before);
* ``ragged_host_ms``: ``align_models`` from host arrays (the common ids, one upload, the gather, the call, the read-back), wall
  clock;
* ``loop_host_ms``: the loop of ``estimate_similarity_with_ransac`` calls on the pairs' items (cut out before the clock
  starts), wall clock;

and their ratios.  Every figure is the median of ``--steps`` timed repetitions after ``--warmup`` (the minimum beside it), the
ragged call and the loop alternating.  The ragged call's outputs are compared with the chains' before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

THR, RMS, ROUNDS = 1e-6, 3, 2


def problem(pairs: int, lo: int, hi: int, seed: int):
    """``align_models``'s arguments: model 0 holds every track, model 1 + q a random subset of n_q of them under a similarity of
    its own (scale 0.5 to 2), noise 3e-4 of its unit per coordinate and 30 % of its points displaced; pair q is (0, 1 + q), its
    threshold THR in the squared unit of model 1 + q."""
    rng = np.random.default_rng(seed)
    world = rng.uniform(-1.0, 1.0, size=(hi, 3))
    points, ids, thr = [world], [np.arange(hi)], []
    for n in rng.integers(lo, hi + 1, pairs):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        angle = rng.uniform(0.2, 2.8)
        W = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
        R = np.eye(3) + np.sin(angle) * W + (1.0 - np.cos(angle)) * (W @ W)
        s = rng.uniform(0.5, 2.0)
        mine = np.sort(rng.permutation(hi)[:n])
        X = s * (world[mine] @ R.T) + rng.uniform(-3.0, 3.0, size=3) + rng.normal(scale=3e-4 * s, size=(n, 3))
        bad = rng.permutation(n)[:int(0.3 * n)]
        X[bad] += s * rng.uniform(-1.0, 1.0, size=(len(bad), 3))
        points.append(X), ids.append(mine), thr.append(THR * s * s)
    return points, ids, np.array([[0, 1 + q] for q in range(pairs)]), np.array(thr)


def _stats(values):
    return sorted(values)[len(values) // 2], min(values)


def time_all(pairs: int, lo: int, hi: int, h: int, steps: int, warmup: int, seed: int, device_only: bool) -> dict:
    import torch

    from structure_from_motion_amd import device
    from structure_from_motion_amd.epipolar.view_graph import pair_min_extra
    from structure_from_motion_amd.multiview.alignment import align_models, common_items, estimate_similarity_with_ransac

    dev = device.require_gpu()
    points, ids, pair_arr, thr = problem(pairs, lo, hi, seed)
    items = [np.hstack([points[i][at_i], points[j][at_j]]) for (i, j), (_, at_i, at_j) in zip(pair_arr.tolist(), common_items(ids, pair_arr))]
    counts = np.array([len(p) for p in items])
    gate = pair_min_extra(counts, 3, 0.25)
    offset = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    items_t, offset_t = device.to_device(np.concatenate(items)), device.to_device(offset, torch.int64)
    thr_t, gate_t = device.to_device(thr), device.to_device(gate.astype(np.float64))
    ws = device.AlignModelsWorkspace(pairs, int(offset[-1]), h, int(counts.max()), dev)
    singles = [(device.SimilarityWorkspace(1, int(n), h, dev), items_t[offset[q]:offset[q + 1]].reshape(1, int(n), 6))
               for q, n in enumerate(counts)]
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def ragged():
        start.record()
        ws.run(items_t, offset_t, thr_t, gate_t, RMS, seed, 1, 0, ROUNDS)
        end.record()
        end.synchronize()
        return start.elapsed_time(end)

    def single():
        total = 0.0
        for q, (one, mine) in enumerate(singles):
            start.record()
            one.run(mine, float(thr[q]), float(gate[q]), RMS, philox=(seed + q, 0, 1))
            one.refine(mine, float(thr[q]), RMS, ROUNDS)
            end.record()
            end.synchronize()
            total += start.elapsed_time(end)
        return total

    # faster and different is not faster: the ragged call's results are the chains'
    ragged(), single()
    status = device.read_align_status(ws.status)
    for q, (one, _) in enumerate(singles):
        if status[q] == device.ALIGN_OK:
            assert torch.equal(ws.model_out[q].view(torch.int64), one.model_out[0].view(torch.int64)), q
            assert torch.equal(ws.mask_out[offset[q]:offset[q + 1]], one.mask_out[0]), q
    for _ in range(warmup):
        ragged(), single()
    t_ragged, t_single = [], []
    for _ in range(steps):
        t_ragged.append(ragged()), t_single.append(single())
    info = device.read_similarity_refine_info(ws.info)
    out = {"pairs": pairs, "items": int(offset[-1]), "items_per_pair": [int(counts.min()), int(counts.max())], "hypotheses": h,
           "refine_rounds": ROUNDS, "calls": steps, "launches_ragged": 7 + 4 * ROUNDS, "launches_loop": pairs * (5 + 4 * ROUNDS),
           "ragged_device_ms": _stats(t_ragged)[0], "ragged_device_min_ms": _stats(t_ragged)[1],
           "single_device_ms": _stats(t_single)[0], "single_device_min_ms": _stats(t_single)[1],
           "pairs_ok": int(np.count_nonzero(status == device.ALIGN_OK)), "rounds_kept": int(sum(r.accepted for r in info)),
           "inliers": int(sum(r.count for r in info))}
    out["device_ratio_single_over_ragged"] = out["single_device_ms"] / out["ragged_device_ms"]
    if device_only:
        return out

    def host_ragged():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        align_models(points, ids, pair_arr, thr, iterations=h, min_num_extra_inliers=3, min_extra_fraction=0.25, refine_rounds=ROUNDS,
                     seed=seed)
        return (time.perf_counter() - t0) * 1e3

    sides = [(np.ascontiguousarray(p[:, :3]), np.ascontiguousarray(p[:, 3:])) for p in items]

    def host_loop():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for q, (a, b) in enumerate(sides):
            estimate_similarity_with_ransac(a, b, float(thr[q]), iterations=h, min_num_extra_inliers=int(gate[q]), refine_rounds=ROUNDS,
                                            seed=seed + q)
        return (time.perf_counter() - t0) * 1e3

    for _ in range(warmup):
        host_ragged(), host_loop()
    h_ragged, h_loop = [], []
    for _ in range(steps):
        h_ragged.append(host_ragged()), h_loop.append(host_loop())
    out.update(ragged_host_ms=_stats(h_ragged)[0], ragged_host_min_ms=_stats(h_ragged)[1], loop_host_ms=_stats(h_loop)[0],
               loop_host_min_ms=_stats(h_loop)[1])
    out["host_ratio_loop_over_ragged"] = out["loop_host_ms"] / out["ragged_host_ms"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--min-items", type=int, default=200)
    ap.add_argument("--max-items", type=int, default=5000)
    ap.add_argument("--hypotheses", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=21, help="timed repetitions of each figure")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--device-only", action="store_true", help="the two device timings only")
    args = ap.parse_args()
    print(json.dumps(time_all(args.pairs, args.min_items, args.max_items, args.hypotheses, args.steps, args.warmup, args.seed,
                              args.device_only)), flush=True)


if __name__ == "__main__":
    main()
