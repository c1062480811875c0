"""Calls of every ``torch.ops.sfm_hip`` op on ``device="meta"`` tensors at tiny sizes: what test_op_meta_fixtures.py reruns
and compares with tests/golden/op_meta_shapes.json (recorded by tests/golden/make_op_fixtures.py before the functional and Meta
forms of each op were merged into one body).  Sizes are pairwise different within a group, so that swapped dimensions show.

A case is ``(id, op name, args)``.  ``functional`` ops get one call per setting of an optional tensor or ``return_*`` flag and
one whose first tensor has the wrong rank (``*/rank``); ``inplace`` ops get one call on correctly shaped buffers."""
import torch

F64, I32, I64, U8 = torch.float64, torch.int32, torch.int64, torch.uint8


def T(*shape, dtype=F64):
    return torch.empty(shape, dtype=dtype, device="meta")


B, N, H = 2, 11, 3                           # batch ops
NT, G, HR = 11, 3, 2                         # ragged ops: offset has G + 1 = 4 entries; HR hypotheses per group
V, HT, W, R, S, D = 3, 5, 7, 2, 2, 4         # dense ops
NZ, NY, NX, TRI = 3, 4, 5, 6                 # TSDF
C, P, M = 3, 5, 11                           # bundle ops and triangulate_tracks
IMG, Q, E, F = 3, 2, 7, 13                   # build_tracks
CAM, EDGE = 3, 4                             # graph solvers
K9 = [800.0, 0.0, 320.0, 0.0, 800.0, 240.0, 0.0, 0.0, 1.0]


def _tables(rows, h, width):
    """S, model, flags, cnt, s1, s2, result of a whole pass over `rows` entries"""
    return [T(rows, h, 8, dtype=I32), T(rows, h, width), T(rows, h, dtype=I32), T(rows, h, dtype=I32), T(rows, h), T(rows, h),
            T(rows, 5, dtype=I64)]


def functional_cases():
    corr, Sb, Eb = T(B, N, 4), T(B, H, 8, dtype=I32), T(B, H, 9)
    record = T(B, 5, dtype=I64)
    pts, model = T(B, N, 5), T(B, H, 12)
    pairs = T(B, N, 6)
    cases = [
        ("normalize_coords", "normalize_coords", (T(B, N, 2), T(B, N, 2), 800.0, 800.0, 320.0, 240.0)),
        ("normalize_coords/rank", "normalize_coords", (T(), T(B, N, 2), 800.0, 800.0, 320.0, 240.0)),
        ("sample_philox", "sample_philox", (5, 0, 0, H, N, B, torch.device("meta"))),
        ("score_sed", "score_sed", (corr, Eb, Sb, 1e-6)),
        ("score_sed/exact", "score_sed", (corr, Eb, Sb, 1e-6, True)),
        ("score_sed/rank", "score_sed", (T(B, N), Eb, Sb, 1e-6)),
        ("select_best", "select_best", (T(B, H, dtype=I32), T(B, H), T(B, H), T(B, H, dtype=I32), 10.0, 3)),
        ("select_best/no_flags", "select_best", (T(B, H, dtype=I32), T(B, H), T(B, H), None, 10.0, 3)),
        ("select_best/rank", "select_best", (T(B, dtype=I32), T(B, H), T(B, H), None, 10.0, 3)),
        ("inlier_mask", "inlier_mask", (corr, Eb, Sb, record, 1e-6)),
        ("inlier_mask/rank", "inlier_mask", (T(B, N), Eb, Sb, record, 1e-6)),
        ("cheirality", "cheirality", (T(N, 4), T(4, 12), 50.0)),
        ("cheirality/rank", "cheirality", (T(N), T(4, 12), 50.0)),
        ("triangulate", "triangulate", (T(N, 4), T(12), T(3, 4))),
        ("triangulate/rank", "triangulate", (T(N), T(12), T(3, 4))),
        ("homography_score", "homography_score", (corr, Eb, Sb, 1e-6)),
        ("homography_score/rank", "homography_score", (T(B, N), Eb, Sb, 1e-6)),
        ("homography_inlier_mask", "homography_inlier_mask", (corr, Eb, Sb, record, 1e-6)),
        ("homography_inlier_mask/rank", "homography_inlier_mask", (T(B, N), Eb, Sb, record, 1e-6)),
        ("pnp_score", "pnp_score", (pts, model, Sb, K9, 1.0)),
        ("pnp_score/rank", "pnp_score", (T(B, N), model, Sb, K9, 1.0)),
        ("pnp_refine", "pnp_refine", (pts, T(B, 12), T(B, N, dtype=U8), T(B), K9, 1.0, 3, 2, 10)),
        ("pnp_refine/rank", "pnp_refine", (T(B, N), T(B, 12), T(B, N, dtype=U8), T(B), K9, 1.0, 3, 2, 10)),
        ("similarity_ransac_pass", "similarity_ransac_pass", (pairs, 5, 0, 0, H, 0.1, 3.0, 3)),
        ("similarity_ransac_pass/rank", "similarity_ransac_pass", (T(B, N), 5, 0, 0, H, 0.1, 3.0, 3)),
        ("similarity_ransac_pass/negative_h", "similarity_ransac_pass", (pairs, 5, 0, 0, -1, 0.1, 3.0, 3)),
        ("similarity_fit", "similarity_fit", (pairs, T(B, N, dtype=U8))),
        ("similarity_fit/no_mask", "similarity_fit", (pairs, None)),
        ("similarity_fit/rank", "similarity_fit", (T(B, N), None)),
        ("similarity_refine", "similarity_refine", (pairs, T(B, 13), T(B, N, dtype=U8), T(B), 0.1, 3, 2)),
        ("similarity_refine/rank", "similarity_refine", (T(B, N), T(B, 13), T(B, N, dtype=U8), T(B), 0.1, 3, 2)),
    ]
    for name in ("fit_eight_point", "five_point_fit", "homography_fit"):
        cases += [(name, name, (corr, Sb)), (name + "/rank", name, (T(B, N), Sb)), (name + "/rank_S", name, (corr, T(B, H, dtype=I32)))]
    for name in ("pnp_fit", "p3p_fit"):
        cases += [(name, name, (pts, Sb, K9)), (name + "/rank", name, (T(B, N), Sb, K9))]

    # ragged ops: with groups and with none
    for tag, groups in (("", G), ("/no_group", 0)):
        offset = T(groups + 1, dtype=I64)
        cases += [
            ("pair_poses" + tag, "pair_poses", (T(NT, 4), offset, T(groups, HR, 9), T(groups, 5, dtype=I64), T(NT, dtype=U8),
                                                T(groups, 3, dtype=I64), 50.0)),
            ("refine_pair_poses" + tag, "refine_pair_poses", (T(NT, 4), offset, T(groups, 128, dtype=U8), 1e-6, 3, 2, 10)),
            ("register_views" + tag, "register_views", (T(NT, 5), offset, T(groups), K9, 5, 0, 0, HR, 1.0, 3, 2, 10)),
            ("align_models" + tag, "align_models", (T(NT, 6), offset, T(groups), T(groups), NT, 5, 0, 0, HR, 3, 2)),
        ]
    offset = T(G + 1, dtype=I64)
    cases += [
        ("pair_poses/rank", "pair_poses", (T(NT), offset, T(G, HR, 9), T(G, 5, dtype=I64), T(NT, dtype=U8), T(G, 3, dtype=I64), 50.0)),
        ("refine_pair_poses/rank", "refine_pair_poses", (T(NT), offset, T(G, 128, dtype=U8), 1e-6, 3, 2, 10)),
        ("register_views/rank", "register_views", (T(NT), offset, T(G), K9, 5, 0, 0, HR, 1.0, 3, 2, 10)),
        ("register_views/no_hypothesis", "register_views", (T(NT, 5), offset, T(G), K9, 5, 0, 0, 0, 1.0, 3, 2, 10)),
        ("register_views/empty_offset", "register_views", (T(NT, 5), T(0, dtype=I64), T(G), K9, 5, 0, 0, HR, 1.0, 3, 2, 10)),
        ("align_models/rank", "align_models", (T(NT), offset, T(G), T(G), NT, 5, 0, 0, HR, 3, 2)),
        ("align_models/no_hypothesis", "align_models", (T(NT, 6), offset, T(G), T(G), NT, 5, 0, 0, 0, 3, 2)),
    ]

    # dense ops
    images, Kt, poses = T(V, HT, W, dtype=U8), T(9), T(V, 12)
    refs, sources, depths = T(R, dtype=I32), T(R, S, dtype=I32), T(R, D)
    volume = T(R, D, HT, W)
    for flag in (False, True):
        cases += [
            (f"plane_sweep/volume={flag}", "plane_sweep", (images, Kt, poses, refs, sources, depths, 2, 2, 1, 1.0, flag)),
            (f"sgm_aggregate/aggregated={flag}", "sgm_aggregate", (volume, depths, 0.1, 0.5, 2.0, 8, flag)),
        ]
    cases += [
        ("plane_sweep/rank", "plane_sweep", (T(V, HT, dtype=U8), Kt, poses, refs, sources, depths, 2, 2, 1, 1.0, False)),
        ("sgm_aggregate/rank", "sgm_aggregate", (T(R, D, HT), depths, 0.1, 0.5, 2.0, 8, False)),
        ("filter_depth_maps", "filter_depth_maps", (T(V, HT, W), Kt, poses, refs, sources, 1.0, 0.01, 1)),
        ("filter_depth_maps/rank", "filter_depth_maps", (T(V, HT), Kt, poses, refs, sources, 1.0, 0.01, 1)),
    ]

    # TSDF: with and without the grey state
    tsum, tcount, views = T(NZ, NY, NX), T(NZ, NY, NX, dtype=I32), T(V, dtype=I32)
    for tag, grey_sum, grey_images in (("", None, None), ("/grey", T(NZ, NY, NX, dtype=I32), images)):
        cases += [
            ("tsdf_integrate" + tag, "tsdf_integrate", (tsum, tcount, grey_sum, T(V, HT, W), grey_images, Kt, poses, views, 0.0, 0.0, 0.0,
                                                        0.1, 0.3)),
            ("tsdf_extract_mesh" + tag, "tsdf_extract_mesh", (tsum, tcount, grey_sum, 0.0, 0.0, 0.0, 0.1, 1, TRI)),
        ]
    cases += [
        ("tsdf_integrate/rank", "tsdf_integrate", (T(NZ, NY), tcount, None, T(V, HT, W), None, Kt, poses, views, 0.0, 0.0, 0.0, 0.1, 0.3)),
        ("tsdf_integrate/rank_views", "tsdf_integrate", (tsum, tcount, None, T(V, HT, W), None, Kt, poses, T(V, 1, dtype=I32), 0.0, 0.0,
                                                          0.0, 0.1, 0.3)),
        ("tsdf_extract_mesh/rank", "tsdf_extract_mesh", (T(NZ, NY), tcount, None, 0.0, 0.0, 0.0, 0.1, 1, TRI)),
        ("tsdf_extract_mesh/negative_triangles", "tsdf_extract_mesh", (tsum, tcount, None, 0.0, 0.0, 0.0, 0.1, 1, -1)),
    ]

    # bundle ops and the tracks
    bposes, bpoints, cam, pt, pixels = T(C, 12), T(P, 3), T(M, dtype=I32), T(M, dtype=I32), T(M, 2)
    for name, extra in (("bundle_adjust", ()), ("bundle_adjust_pcg", (50, 0.1)), ("bundle_adjust_robust", (1, 2.0)),
                        ("bundle_adjust_pcg_robust", (50, 0.1, 1, 2.0)), ("bundle_adjust_calibrated", (1, 2.0, 3))):
        cases += [(name, name, (bposes, bpoints, cam, pt, pixels, K9, [0], 10) + extra),
                  (name + "/rank", name, (T(C), bpoints, cam, pt, pixels, K9, [0], 10) + extra)]
    cases += [
        ("triangulate_tracks", "triangulate_tracks", (bposes, cam, pt, pixels, P, K9, 2, 0.01, 4.0, 5)),
        ("triangulate_tracks/rank", "triangulate_tracks", (T(C), cam, pt, pixels, P, K9, 2, 0.01, 4.0, 5)),
        ("build_tracks", "build_tracks", (T(IMG + 1, dtype=I32), T(Q, 2, dtype=I32), T(Q + 1, dtype=I32), T(E, 2, dtype=I32), F)),
        ("build_tracks/rank", "build_tracks", (T(IMG + 1, 1, dtype=I32), T(Q, 2, dtype=I32), T(Q + 1, dtype=I32), T(E, 2, dtype=I32), F)),
    ]

    # graph solvers: `initial` (and the translations' `rotations`) given and None
    gpairs, weights = T(EDGE, 2, dtype=I32), T(EDGE)
    limits = (1, 0.1, 20, 50, 0.1, 1e-9)
    for tag, initial in (("", None), ("/initial", T(CAM, 3, 3))):
        cases.append(("average_rotations" + tag, "average_rotations", (gpairs, T(EDGE, 9), weights, CAM, 0, initial) + limits))
    cases.append(("average_rotations/rank", "average_rotations", (T(EDGE, dtype=I32), T(EDGE, 9), weights, CAM, 0, None) + limits))
    tlimits = (1, 0.1, 5, 20, 50, 0.1, 1e-9)
    for tag, rotations, initial in (("", None, None), ("/initial", None, T(CAM, 3)), ("/rotations", T(CAM, 9), None)):
        cases.append(("average_translations" + tag, "average_translations", (gpairs, T(EDGE, 3), rotations, weights, CAM, 0, initial) + tlimits))
    cases.append(("average_translations/rank", "average_translations", (T(EDGE, dtype=I32), T(EDGE, 3), None, weights, CAM, 0, None) + tlimits))
    return cases


def inplace_cases():
    corr, Sb, Eb = T(B, N, 4), T(B, H, 8, dtype=I32), T(B, H, 9)
    one, S1, E1 = T(1, N, 4), T(1, H, 8, dtype=I32), T(1, H, 9)
    bh_i, bh_d = T(B, H, dtype=I32), T(B, H)
    record, mask = T(B, 5, dtype=I64), T(B, N, dtype=U8)
    pts = T(B, N, 5)
    cases = [
        ("normalize_coords_", (T(B, N, 2), T(B, N, 2), 800.0, 800.0, 320.0, 240.0, corr)),
        ("fit_eight_point_", (corr, Sb, Eb, bh_i)),
        ("five_point_fit_", (corr, Sb, Eb, bh_i)),
        ("sample_fit_philox_", (corr, 5, None, 0, 0, Sb, Eb, bh_i)),
        ("score_sed_", (corr, Eb, Sb, 1e-6, bh_i, bh_d, bh_d, None)),
        ("select_best_", (bh_i, bh_d, bh_d, bh_i, 10.0, 3, 0, record)),
        ("inlier_mask_", (corr, Eb, Sb, record, 1e-6, mask)),
        ("five_point_ransac_pass_", (corr, 5, 0, True, 0, 1e-6, 10.0, 3, *_tables(B, H, 9), mask)),
        ("homography_ransac_pass_", (corr, 5, 0, True, 0, 1e-6, 10.0, 3, *_tables(B, H, 9), None)),
        ("similarity_ransac_pass_", (T(B, N, 6), 5, 0, True, 0, 0.1, 3.0, 3, *_tables(B, H, 13), mask)),
        ("pnp_fit_", (pts, Sb, K9, T(B, H, 12), bh_i)),
        ("p3p_fit_", (pts, Sb, K9, T(B, H, 12), bh_i)),
        ("pnp_score_", (pts, T(B, H, 12), Sb, K9, 1.0, bh_i, bh_d, bh_d)),
        ("pnp_ransac_pass_", (pts, 5, 0, True, 0, K9, 1.0, 10.0, 3, *_tables(B, H, 12), mask)),
        ("p3p_ransac_pass_", (pts, 5, 0, True, 0, K9, 1.0, 10.0, 3, *_tables(B, H, 12), None)),
        ("pnp_refine_", (pts, T(B, 12), mask, T(B), K9, 1.0, 3, 2, 10, T(B, 12), T(B, N, dtype=U8), T(B, 3, dtype=I64))),
        ("similarity_fit_", (T(B, N, 6), mask, T(B, 13), T(B, dtype=I32))),
        ("similarity_refine_", (T(B, N, 6), T(B, 13), mask, T(B), 0.1, 3, 2, T(B, 13), T(B, N, dtype=U8), T(B, 3, dtype=I64))),
    ]
    for name in ("ransac_pass_small_", "ransac_pass_large_"):
        cases.append((name, (one, 5, None, True, 0, 1e-6, 10.0, 3, 0, *_tables(1, H, 9), T(1, N, dtype=U8), T(64, dtype=U8))))

    offset = T(G + 1, dtype=I64)
    gh_i, gh_d = T(G, HR, dtype=I32), T(G, HR)
    cases += [
        ("verify_pairs_", (T(NT, 4), offset, T(G), 5, 0, 0, 1e-6, 3, 0.8, T(G, HR, 8, dtype=I32), T(G, HR, 9), T(G, HR, 9), gh_i, gh_i,
                           gh_d, gh_d, gh_i, gh_i, gh_d, gh_d, T(G, 5, dtype=I64), T(G, 5, dtype=I64), T(NT, dtype=U8), T(NT, dtype=U8),
                           T(G, 3, dtype=I64))),
        ("register_views_", (T(NT, 5), offset, T(G), K9, 5, 0, 0, 1.0, 3, 2, 10, *_tables(G, HR, 12), T(NT, dtype=U8), T(G, 12),
                             T(NT, dtype=U8), T(G, 3, dtype=I64), T(G, dtype=I32))),
        ("align_models_", (T(NT, 6), offset, T(G), T(G), NT, 5, 0, 0, 3, 2, *_tables(G, HR, 13), T(NT, dtype=U8), T(G, 13),
                           T(NT, dtype=U8), T(G, 3, dtype=I64), T(G, dtype=I32))),
    ]

    images, Kt, poses = T(V, HT, W, dtype=U8), T(9), T(V, 12)
    refs, sources, depths = T(R, dtype=I32), T(R, S, dtype=I32), T(R, D)
    rhw_d, rhw_i = T(R, HT, W), T(R, HT, W, dtype=I32)
    tsum, tcount = T(NZ, NY, NX), T(NZ, NY, NX, dtype=I32)
    cases += [
        ("plane_sweep_", (images, Kt, poses, refs, sources, depths, 2, 2, 1, 1.0, rhw_d, rhw_i, rhw_d, T(R, dtype=I32), T(R, D, HT, W))),
        ("filter_depth_maps_", (T(V, HT, W), Kt, poses, refs, sources, 1.0, 0.01, 1, rhw_i, rhw_d, T(R, HT, W, 3), T(R, dtype=I32))),
        ("sgm_aggregate_", (T(R, D, HT, W), depths, 0.1, 0.5, 2.0, 8, rhw_d, rhw_i, rhw_d, None)),
        ("tsdf_integrate_", (tsum, tcount, None, T(V, HT, W), None, Kt, poses, T(V, dtype=I32), 0.0, 0.0, 0.0, 0.1, 0.3, T(V, dtype=I32))),
        ("tsdf_extract_mesh_", (tsum, tcount, None, 0.0, 0.0, 0.0, 0.1, 1, T(TRI, 3, 3), None, T(1, dtype=I64))),
    ]

    bposes, bpoints, cam, pt, pixels = T(C, 12), T(P, 3), T(M, dtype=I32), T(M, dtype=I32), T(M, 2)
    head = (bposes, bpoints, cam, pt, pixels, K9, [0], 10)
    f_i = T(F, dtype=I32)
    cases += [
        ("bundle_adjust_", head + (T(4, dtype=I64),)),
        ("bundle_adjust_pcg_", head + (50, 0.1, T(5, dtype=I64))),
        ("bundle_adjust_robust_", head + (1, 2.0, T(4, dtype=I64))),
        ("bundle_adjust_pcg_robust_", head + (50, 0.1, 1, 2.0, T(5, dtype=I64))),
        ("bundle_adjust_calibrated_", head + (1, 2.0, 3, T(4, dtype=I64), T(3, 3))),
        ("triangulate_tracks_", (bposes, cam, pt, pixels, P, K9, 2, 0.01, 4.0, 5, T(P, 3), T(P, dtype=U8), T(M), T(P), T(4, dtype=I64))),
        ("build_tracks_", (T(IMG + 1, dtype=I32), T(Q, 2, dtype=I32), T(Q + 1, dtype=I32), T(E, 2, dtype=I32), F, f_i, f_i,
                           T(F, dtype=U8), f_i, f_i, f_i, T(6, dtype=I64))),
    ]
    return [(name, name, args) for name, args in cases]


def schemas():
    """name (with its overload) -> str(schema) of every registered ``sfm_hip::`` op"""
    found = {}
    for schema in torch._C._jit_get_all_schemas():
        if schema.name.startswith("sfm_hip::"):
            found[schema.name + ("." + schema.overload_name if schema.overload_name else "")] = str(schema)
    return found


def outcome(op, name, args):
    """What a call gives: None, the list of [shape, dtype] of its outputs, or {"error": text}.  Where torch itself refuses a
    negative size, the text stops before the sizes: they are those of whichever output the op allocates first."""
    try:
        out = getattr(op, name)(*args)
    except Exception as e:   # noqa: BLE001  (the text is the point, whatever the type)
        text = str(e).split("\nException raised from")[0]
        negative = "Trying to create tensor with negative dimension"
        return {"error": negative if text.startswith(negative) else text}
    if out is None:
        return None
    return [[list(t.shape), str(t.dtype)] for t in (out if isinstance(out, (tuple, list)) else (out,))]


def run(op):
    """id -> outcome of every case"""
    return {case: outcome(op, name, args) for case, name, args in functional_cases() + inplace_cases()}
