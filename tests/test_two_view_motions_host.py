"""The two-view definitions on the host over the family of relative motions in tests/motion_cases.py: the five-point solver
(structure_from_motion_amd/epipolar/five_point.py) against the true E and the action-matrix oracle, and the eight-point
oracle's own chain (fit, decomposition, cheirality vote), which the GPU tests of the same motions compare against.
No GPU needed.

Figures in the comments come from ``pytest tests/test_two_view_motions_host.py -s``, which prints every one of them."""
import itertools

import numpy as np
import pytest

import five_point_oracle as fpo
import motion_cases as mc
from oracle import sfm_oracle as orc
from structure_from_motion_amd.epipolar import five_point as fp

N = 200
SCENE_SEED = 1


def _truth_gap(E, Et):
    """max |E - (+-)Et| over the last axis: the true E in either sign (mc.unit_gap says why)."""
    return np.minimum(np.abs(E - Et).max(axis=-1), np.abs(E + Et).max(axis=-1))


@pytest.mark.parametrize("motion", mc.NAMES)
def test_five_point_recall(motion):
    """The floors of test_five_point_host.test_true_essential_is_a_candidate on every motion, the true E taken in either
    sign.  Before the null basis was mixed and the candidates polished the shares within 1e-9 / 1e-6 on
    these samples were: roll10_tx 0.962 / 0.963 (3.7 % of the samples without a candidate), tz 0.742 / 0.962, gen_tz
    0.736 / 0.952, roll180_tx 0.965 / 0.965 (3.4 % without), roll15_tz 0.696 / 0.949, tx 0.922 / 0.926 (7.4 % without),
    roll90_tx 0.000 / 0.000, and 0.950 / 0.993 or better on the eight others.  Now: tz 0.997 / 0.998, gen_tz 0.995 / 0.997,
    roll15_tz 0.997 / 0.998, every other motion 1.000 / 1.000, no sample without a candidate."""
    sc = mc.scene(motion, N, SCENE_SEED)
    S = mc.samples(N, 1000, 6, 2)
    Et = mc.true_essential(sc["R"], sc["t"])
    pts = sc["corr"][S]
    cands, count, degenerate, _ = fp.solve(pts[:, :5, 0:2], pts[:, :5, 2:4])
    assert not degenerate.any()
    err = np.min(np.where(np.isnan(cands[:, :, 0]), np.inf, _truth_gap(cands, Et)), axis=1)
    E, flags = fp.fit_corr(sc["corr"], S)
    assert not flags.any()
    with np.errstate(invalid="ignore"):
        pick = np.where(np.isnan(E[:, 0]), np.inf, _truth_gap(E, Et))
    print(f"{motion}: within 1e-9 {np.mean(err <= 1e-9):.3f}, within 1e-6 {np.mean(err <= 1e-6):.3f}, no candidate "
          f"{np.mean(count == 0):.3f}, item 5 picks it {np.mean(pick <= 1e-6):.3f}")
    assert np.mean(err <= 1e-9) >= 0.94
    assert np.mean(err <= 1e-6) >= 0.98
    assert np.mean(pick <= 1e-6) >= 0.98


@pytest.mark.parametrize("motion", mc.NAMES)
def test_action_matrix_oracle_is_a_reference(motion):
    """The action-matrix oracle also fixes the coefficient of its fourth null vector to 1, so it could lose the solution
    where the solver did.  It does not: its null basis comes from an SVD, whose last vector has no reason to be orthogonal
    to the true E.  Measured: it has the true E within 1e-6 on 100 of 100 samples of every motion but roll10_tx (99: one
    sample's 10 x 10 block is singular to LAPACK), so it is a reference for the true solution on every motion, and the
    solver must have the true E wherever the oracle has it, at the floor of test_true_essential_is_a_candidate.

    It is no reference for the other candidates on tx, roll10_tx, roll90_tx and roll180_tx: there the two solvers return
    different numbers of them (equal on 34 to 40 of 100 samples, the difference always even) although each one's
    candidates satisfy the constraints to 1e-13.  The other solutions of these motions are double roots, which rounding
    splits into a real or a complex pair in each solver.  The counts are printed, not asserted; on the eleven other
    motions they agree on 99 or 100 samples."""
    sc = mc.scene(motion, N, SCENE_SEED)
    S = mc.samples(N, 100, 6, 2)
    Et = mc.true_essential(sc["R"], sc["t"])
    pts = sc["corr"][S]
    cands, count, _, _ = fp.solve(pts[:, :5, 0:2], pts[:, :5, 2:4])
    hit = both = agree = close = 0
    for i in range(len(S)):
        try:
            ref = fpo.solve(pts[i, :5, 0:2], pts[i, :5, 2:4])
        except np.linalg.LinAlgError:
            continue
        has = bool(ref) and min(_truth_gap(e, Et) for e in ref) <= 1e-6
        hit += has
        both += has and count[i] > 0 and np.min(_truth_gap(cands[i, :count[i]], Et)) <= 1e-6
        agree += len(ref) == count[i]
        if len(ref) == count[i]:
            close += (max(np.min(_truth_gap(cands[i, :count[i]], e)) for e in ref) if ref else 0.0) <= 1e-6
    print(f"{motion}: the oracle has the true E on {hit} of 100, the solver too on {both}; counts agree on {agree}, every "
          f"candidate on {close}")
    assert hit >= 98
    assert both >= 0.98 * hit


@pytest.mark.parametrize("motion", mc.NAMES)
def test_eight_point_oracle_chain(motion):
    """orc.fit_hypotheses -> orc.recover_all_r_t -> orc.cheirality_pass on noise-free samples: what the device's eight-point
    fit, decomposition and vote are compared with on the GPU.

    On every motion with E[2][2] = 0 the fitted E / E[2][2] has a magnitude of 1e12 .. 1e19 (median 3e13), and its third
    singular value, 2e-17 of the first (largest 4e-16 over all motions), is then 1e-9 .. 1 in absolute terms:
    recover_all_r_t's np.isclose(0, s[-1]), absolute like the reference's, refuses 462 to 499 of 500 such fits.  The pose
    does not depend on the scale of E, so the chain is run on mc.unit(E), which is what the GPU tests do too.

    Measured over 500 samples per motion (sample seed 3): at most 0.2 % flagged, at most 0.2 % of the unflagged fits not
    finite; largest SED over the 200 points: 99th percentile at most 1.5e-15 (turn170; 1e-17 or less elsewhere), median at
    most 1.4e-22 (by hand on other samples: 1.1e-16 and 1.3e-22).  The caps are ten times the larger of the two figures.
    Every unflagged finite fit goes through the decomposition and the vote."""
    sc = mc.scene(motion, N, SCENE_SEED)
    corr = sc["corr"]
    S = mc.samples(N, 500, 8, 3)
    E, flagged, _ = orc.fit_hypotheses(corr, S)
    finite = np.isfinite(E).all(axis=(1, 2))
    not_finite = np.mean(~finite[~flagged])
    ok = ~flagged & finite
    sed = orc.sed_values(E[ok], corr).max(axis=1)
    print(f"{motion}: flagged {flagged.mean():.3f}, unflagged and not finite {not_finite:.3f}, largest SED p99 "
          f"{np.quantile(sed, 0.99):.1e} median {np.median(sed):.1e}, |E| median {np.median(np.abs(E[ok]).max(axis=(1, 2))):.1e}")
    assert flagged.mean() < 0.01 and not_finite < 0.01      # a condition on the samples: change the seed, not the cap
    assert np.quantile(sed, 0.99) <= 1.5e-14 and np.median(sed) <= 1.4e-21
    t_true = sc["t"] / np.linalg.norm(sc["t"])
    Et = mc.true_essential(sc["R"], sc["t"])
    for e in E[ok]:
        R1, R2, t1 = orc.recover_all_r_t(mc.unit(e))
        poses = list(itertools.product([R1, R2], [t1, -t1]))
        votes = [int(orc.cheirality_pass(corr, R, t).sum()) for R, t in poses]
        assert sorted(votes) == [0, 0, 0, N], votes
        R, t = poses[int(np.argmax(votes))]
        # a perturbation d of E (sigma = 1, 1, 0: unit gaps between the singular values) turns its singular vectors, and
        # with them R and t, by a small multiple of d
        bound = 10.0 * float(mc.unit_gap(e, Et.reshape(3, 3))) + 1e-12
        assert np.abs(R - sc["R"]).max() <= bound and np.abs(t - t_true).max() <= bound, (bound, np.abs(R - sc["R"]).max())


def test_unit_and_scene():
    E = np.array([[0.0, -3.0, 1.0], [3.0, 0.0, -2.0], [-1.0, 2.0, 0.0]])
    for scale in (1.0, -1e16, 1e-16, 1e200, -1e-200):
        u = mc.unit(scale * E)
        assert abs(np.linalg.norm(u) - np.sqrt(2.0)) <= 1e-15 and u.reshape(9)[np.argmax(np.abs(u))] > 0
        assert mc.unit_gap(scale * E, E) <= 1e-15
    assert np.isnan(mc.unit(np.where(np.eye(3) > 0, np.nan, E))).all()
    assert np.isnan(mc.unit(np.full(9, np.inf))).all()
    assert mc.unit(np.stack([E, 2 * E]).reshape(2, 9)).shape == (2, 9)
    for motion in mc.NAMES:
        R, t = mc.MOTIONS[motion]
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(R) - 1.0) <= 1e-15
        sc = mc.scene(motion, 300, 4, noise_px=0.5, outlier_fraction=0.25)
        assert 40 <= sc["is_outlier"].sum() <= 110
        clean = mc.scene(motion, 300, 4)
        inl = ~sc["is_outlier"]
        assert 0.1 <= np.abs(sc["pix_b"][inl] - clean["pix_b"][inl]).std() <= 1.0     # 0.5 px of noise, in pixels
        Et = mc.true_essential(R, t).reshape(3, 3)
        assert orc.sed_values(Et, clean["corr"]).max() <= 1e-28
        assert np.array_equal(clean["corr"][:, 0], (clean["pix_a"][:, 0] - sc["K"][0, 2]) / sc["K"][0, 0])
