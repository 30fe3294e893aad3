"""The map-point kernels of the pose-update chain at the camera counts that change their lane layout (coslam_amd/csrc/poseupdate.hip):

  check_unify_wave (k_check_unify)       LPP lanes per (camera, point) pair: 8 up to 4 cameras, 4 at 5-8, 2 at 9-16
  cls_is_static (k_map_points_classify)  LPC lanes per camera: 8 up to 8 cameras, 4 at 9-16
  chain_widest_w                         the group-wide reduction of both, W = LPP / LPC: strides over the chain, nearest node among equals
  up_point (k_update_points)             camera c's two views in lane c, the Jacobian blocks summed by shuffle over nCams lanes

against the reference's own code at 7, 8, 9, 12 and 13 cameras (tests/golden/*_wide*_golden.npz, made by tests/cxx/ref_update_points_test.cpp
and ref_classify_test.cpp golden_wide / golden_wide_relink) and against the oracle at 14 and 16 (tests/poseupdate_wide_scenes.py; the
reference stops at 13, and tests/test_oracle_cpu.py holds the oracle to the reference at 7..13).  Everything bit for bit: the launch
loops are those of tests/test_poseupdate_gpu.py (tests/poseupdate_golden_dev.py).  tests/test_oracle_cpu.py asserts from the fixtures alone
what the width statements below rely on (fully seen points, chain lengths, pairs with 4 * nCams views)."""
import os

import numpy as np
import pytest

from tests.poseupdate_golden_dev import check_unify_on, classify_on, classify_refs_on, relink_chains_on, update_points_on

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_update_and_refine_map_points_at_7_to_13_cameras():
    """cs_update_new_poses_points_dev and cs_refine_map_points_dev (k_update_points / up_point) on update_points_wide_golden.npz: 7 cameras
    moving, 8 and 9 standing still for the older half of the history (equal cosines: the wave-wide reduction's tie-break, W = 64), 12
    rotation only, 13 moving; 12-15 points per scene with both views of EVERY camera, so the covariance tail shuffles from lanes 0..nCams-1
    all holding two Jacobians.  Points, covariances and counts equal the reference's (187 of 240 points re-triangulated, 238 refined)."""
    assert update_points_on(np.load(os.path.join(GOLD, "update_points_wide_golden.npz"))) == 187


def test_check_unify_at_7_to_13_cameras():
    """cs_check_unify_dev (k_check_unify / check_unify_wave) on the 521 pairs of update_points_wide_golden.npz: LPP = 4 at 7 and 8 cameras --
    at 8 the 16 (camera, point) pairs occupy all 64 lanes in the 13 pairs of two fully seen points --, LPP = 2 at 9, 12 and 13 (52 of 64
    lanes, 52 views: the reference's limit).  The stand-still scenes (8: LPP 4, 9: LPP 2) decide the group reduction's tie-break; the
    12-camera rig only rotates (no second views, NaN-free here).  Verdict, M and cov equal the reference's; 234 pairs unify."""
    assert check_unify_on(np.load(os.path.join(GOLD, "update_points_wide_golden.npz"))) == (521, 234)


def test_relinked_chains_at_8_and_13_cameras():
    """cs_update_new_poses_points_ref_dev, cs_refine_map_points_ref_dev, cs_feat_ref_advance_refine_dev and cs_check_unify_ref_dev over
    featRef / segPool on update_points_wide_relink_golden.npz (chains with stale heads and segments linked behind, up to 51 nodes):
    k_update_points with a wave per point, k_check_unify with LPP = 4 and all 64 lanes occupied at 8 cameras (pairs of two fully seen
    points), LPP = 2 and 52 lanes at 13, whose rig stands still for the older half of its 70 frames (equal cosines behind
    links: the tie-break at W = 2 and W = 64) -- the groups' strides cross segment boundaries."""
    assert relink_chains_on(np.load(os.path.join(GOLD, "update_points_wide_relink_golden.npz"))) == (62, 211)


def test_map_points_classify_at_8_9_and_13_cameras():
    """cs_map_points_classify_dev (k_classify_select, k_map_points_classify / cls_is_static) on classify_wide_golden.npz: LPC = 8 over 8
    cameras -- all 64 lanes occupied for the 26 points every camera sees --, LPC = 4 at 9 (36 lanes; every third camera stood still for the
    older half of its history: equal cosines in the window) and at 13 cameras (52 lanes); chains up to 63 nodes against isStaticPoint's
    window of 60.  Every output array of the 3-5 camera test; 44 of a scene's 48 points are looked at."""
    assert classify_on(np.load(os.path.join(GOLD, "classify_wide_golden.npz")), min_examined=40) > 120


def test_map_points_classify_over_feature_references_at_8_and_13_cameras():
    """The same behind cs_track_history_set_classify_refs on classify_wide_relink_golden.npz (862 chains, 151 stale heads, 597 linked):
    LPC = 8 with all 64 lanes occupied at 8 cameras, LPC = 4 at 13, the groups walking through linked segments; with the table at this
    frame and one frame behind.  (The detached views of this fixture are live ones: no stale view is detached.)"""
    examined, stale_detached = classify_refs_on(np.load(os.path.join(GOLD, "classify_wide_relink_golden.npz")), min_examined=40)
    assert examined > 75 and stale_detached == 0


def test_map_point_kernels_at_14_and_16_cameras_equal_the_oracle():
    """All of the above on the 14- and 16-camera scenes of tests/poseupdate_wide_scenes.py, the oracle's output as the expectation: at 16
    cameras LPP = 2 over 32 (camera, point) pairs and LPC = 4 over 16 cameras occupy all 64 lanes, and a pair of two fully seen points
    puts its 64th view into check_unify_wave's flat rotation array (7 such pairs a scene); at 14, 56 lanes.  Every odd camera stood still
    (tie-breaks at W = 2, 4 and 64), chains are up to 40 nodes long over a ring of 32 frames: the walk bound cuts them."""
    from tests.poseupdate_wide_scenes import classify_ref_scenes, classify_scenes, update_scenes

    g = update_scenes()
    expect = sum(int((g[f"s{sc}_M_ref"] != g[f"s{sc}_M0"]).any(axis=1).sum()) for sc in range(int(g["n_scenes"])))
    assert update_points_on(g) == expect >= 30
    n_all, n_yes = check_unify_on(g)
    assert n_all >= 100 and 4 * n_yes >= n_all and 4 * (n_all - n_yes) >= n_all
    assert relink_chains_on(g) == (expect, n_all)
    assert classify_on(classify_scenes(), min_examined=8) >= 20
    assert classify_refs_on(classify_ref_scenes(), min_examined=8, differs_without_refs=False)[0] >= 20
