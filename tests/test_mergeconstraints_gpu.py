"""cs_merge_constraints_assemble_dev on the device (Stage A) against the reference's own genMergeInfoVer2
(tests/golden/mergeconstraints_golden.npz) bit for bit, and -- where the reference cannot go: an empty or wholly skipped match list, fewer
than three views, 16 cameras (its SLAM_MAX_NUM is 13), more tracks than one pass of the workgroup -- against the restatement
tests/mergeconstraints_ref.py, which the CPU tests pin to the same file."""
import os

import numpy as np
import pytest

import coslam_amd
from tests import mergeconstraints_ref as ref
from tests.mergeconstraints_dev import DeviceScene, assemble_dev, same_problem
from tests.mergeconstraints_golden_util import expand, load
from tests.mergeconstraints_scenes import make_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = load()


def _dev():
    import torch

    return torch.device("cuda:0")


def _make_scene(spec, seed):
    S = expand(make_scene(0, spec, np.random.default_rng(seed)))
    ids = ref.cam_ids_in_both_groups(S["groups"], S["gId1"], S["gId2"])
    return S, int(S["key_frames"][ref.first_constrain(S["key_frames"], S["self_motion"], ids)[0]])


def _views_equal(views, A):
    assert views.tolist() == [[int(x) for x in v] for v in A["views"]]


@pytest.mark.parametrize("sc", range(len(SCENES)))
def test_assemble_equals_the_reference(hip, sc):
    """every scene of the golden file, the handle created for exactly the scene's matches and map rows: header, poses, points, pointMap,
    obs_ptr / obs_cam / obs_xy and avgErr bit for bit; the merge list applied gives the recorded post-state; no input table changes"""
    S, G = SCENES[sc]
    D = DeviceScene(S, _dev())
    before = D.snapshot()
    mc, P, views = assemble_dev(D, int(G["first_frame"]))
    after = D.snapshot()
    for k in before:
        assert np.array_equal(before[k], after[k]) and before[k].tobytes() == after[k].tobytes(), k
    h = P["header"]
    assert (h.verdict, h.avgErr, h.f1, h.f2) == (int(G["verdict"]), float(G["avgErr"]), int(G["first_frame"]), S["frame0"] + S["nF"] - 1)
    assert [(int(G["order"][i][0]), h.camIds[i % h.nCamIds]) for i in range(len(G["order"]))] == [tuple(int(v) for v in r) for r in G["order"]]
    if h.verdict == 1:
        assert (h.nPose, h.P, h.nObs) == (len(G["order"]), len(G["pts"]), len(G["obs_cam"]))
        for k in ("Ks", "Rs", "Ts", "pts", "obs_xy"):
            assert np.array_equal(P[k], G[k]), k
        for k, g in (("pointMap", "pointMap"), ("obs_ptr", "obs_ptr"), ("obs_cam", "obs_cam")):
            assert np.array_equal(P[k], G[g].astype(np.int32)), k
    A = ref.assemble(S, int(G["first_frame"]))
    same_problem(P, A)
    _views_equal(views, A)
    cur, pfeat, det = ref.apply_views(S, views.tolist(), int(G["first_frame"]))
    assert np.array_equal(np.array(cur), G["cur_mpt"]) and np.array_equal(np.array(pfeat), G["pfeat"])
    assert [list(d) for d in det] == sorted(G["detached"].tolist())
    mc.close()
    D.th.close()


def test_planted_match_lists(hip):
    """K = 0; every match skipped (a slot outside the table, a slot that is no feature, a feature of no map point); a single match whose
    track has two views: CS_MERGE_FEW and nothing produced, never a read outside a table"""
    S, G = SCENES[0]
    f1, N = int(G["first_frame"]), S["N"]
    D = DeviceScene(S, _dev())
    iC, jC = S["maxiCam"], S["maxjCam"]
    untracked_i = int(np.nonzero(~np.isin(S["state"][iC], (0, 1)))[0][0])
    unmapped_j = int(np.nonzero(np.isin(S["state"][jC], (0, 1)) & (S["slot2map"][jC] < 0))[0][0])
    good = [int(v) for v in S["matches"][0]]
    skipped = [[-1, good[1]], [good[0], N], [N + 5000, -7], [untracked_i, good[1]], [good[0], unmapped_j], [2 ** 30, 2 ** 30]]
    for m, n_skip in (([], 0), (skipped, len(skipped))):
        mc, P, views = assemble_dev(D, f1, matches=m, max_matches=max(1, len(m)))
        A = ref.assemble(dict(S, matches=np.array(m, np.int32).reshape(-1, 2)), f1)
        assert A["verdict"] == ref.VERDICT_FEW and A["skipped"] == n_skip
        same_problem(P, A)
        assert len(views) == 0
        mc.close()
    two = None
    for a, b in S["matches"]:
        A = ref.assemble(dict(S, matches=np.array([[a, b]], np.int32)), f1)
        if A["nMergedTracks"] == 1 and A["verdict"] == ref.VERDICT_FEW:
            two = [[int(a), int(b)]]
            break
    assert two is not None, "no match of the scene has a track of two views"
    mc, P, _ = assemble_dev(D, f1, matches=two)
    same_problem(P, ref.assemble(dict(S, matches=np.array(two, np.int32)), f1))
    assert P["header"].verdict == -1 and P["header"].nMergedTracks == 1
    mc.close()
    D.th.close()


def test_verdict_on_either_side_of_500(hip):
    """the first merged point moved along x until the mean of the three largest errors stands just below and just above the threshold"""
    S, G = SCENES[3]
    f1 = int(G["first_frame"])
    m1 = int(S["slot2map"][S["maxiCam"]][int(S["matches"][0][0])])
    base = S["M"].copy()

    def scene(dx):
        M = base.copy()
        M[m1, 0] += dx
        return dict(S, M=M)

    lo, hi = 0.0, 64.0
    assert ref.assemble(scene(hi), f1)["avgErr"] > 500 > ref.assemble(scene(lo), f1)["avgErr"]
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if ref.assemble(scene(mid), f1)["avgErr"] <= 500 else (lo, mid)
    for dx, verdict in ((lo, 1), (hi, 0)):
        Sx = scene(dx)
        A = ref.assemble(Sx, f1)
        assert A["verdict"] == verdict and abs(A["avgErr"] - 500) < 1e-6
        D = DeviceScene(Sx, _dev())
        mc, P, _ = assemble_dev(D, f1)
        same_problem(P, A)
        mc.close()
        D.th.close()


def test_refusals_before_any_launch(hip):
    """f1 outside the store, f1 not behind f2, f2 not the newest frame, more matches than the handle holds: CS_ERR_INVALID, and the header
    of an earlier run still stands"""
    S, G = SCENES[4]
    f1, f2 = int(G["first_frame"]), S["frame0"] + S["nF"] - 1
    D = DeviceScene(S, _dev(), hist_len=8, store_len=8)           # the store holds the newest 8 of 16 frames: f1 has left it
    assert f2 - f1 >= 8
    mc = coslam_amd.MergeConstraints(S["nC"], S["N"], len(S["matches"]), S["nMap"])
    args = (D.th, D.cams, D.featRef.data_ptr(), S["nMap"], D.M.data_ptr(), D.groups.data_ptr(), S["gId1"], S["gId2"], S["maxiCam"], S["maxjCam"])
    ok_f1 = f2 - 3
    mc.assemble(*args, ok_f1, f2, S["matches"])
    h0 = bytes(mc.header())
    for bad_f1, bad_f2, m, what in ((f1, f2, S["matches"], "store"), (f2 - 8, f2, S["matches"], "store"), (f2, f2, S["matches"], "behind"),
                                    (ok_f1, f2 - 1, S["matches"], "newest"), (ok_f1, f2, np.tile(S["matches"], (2, 1)), "created for")):
        with pytest.raises(coslam_amd.CoslamHipError, match=what):
            mc.assemble(*args, bad_f1, bad_f2, m)
        assert bytes(mc.header()) == h0
    with pytest.raises(coslam_amd.CoslamHipError):
        mc.assemble(*args[:6], S["gId1"], S["gId1"], S["maxiCam"], S["maxjCam"], ok_f1, f2, S["matches"])
    mc.assemble(*args[:6], 5, S["gId2"], S["maxiCam"], S["maxjCam"], ok_f1, f2, S["matches"])     # a group the record does not hold
    assert mc.header().verdict == -2 and mc.header().nPose == 0
    mc.close()
    D.th.close()


def test_sixteen_cameras_and_many_tracks(hip):
    """two groups of 8 (more slots than one pass of the workgroup), and a scene with more tracks than lanes: against the restatement"""
    specs = (dict(groups=[[0, 3, 1, 2, 4, 7, 6, 5], [8, 9, 15, 14, 13, 12, 11, 10]], g=(1, 0), ij=(12, 3), nF=12, gaps=(2, 3, 4),
                  moved=[{1, 9}, set(), set(range(16))], nA=60, nB=60, nMatch=14, plant="shared"),
             dict(groups=[[0, 1], [3, 2]], g=(0, 1), ij=(1, 3), nF=10, gaps=(3, 2, 2), moved=[{0, 1, 2, 3}, {1}, set()], nA=700, nB=700, nMatch=64,
                  plant="mixed"))
    for k, spec in enumerate(specs):
        S, f1 = _make_scene(spec, 300 + k)
        A = ref.assemble(S, f1)
        assert A["verdict"] == 1
        if k == 0:
            assert S["nC"] == 16 and len(A["cam_ids"]) == 16 and len(A["cam_ids"]) * S["N"] > 1024 and max(A["obs_cam"]) == 31
        else:
            assert A["nMergedTracks"] + A["nUnmerged"] > 1024 and len(S["matches"]) > 64
        D = DeviceScene(S, _dev())
        mc, P, views = assemble_dev(D, f1)
        same_problem(P, A)
        _views_equal(views, A)
        mc.close()
        D.th.close()
