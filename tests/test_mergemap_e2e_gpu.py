"""coslam_amd.MergeCamGroups: "matches in, merged state out" as one call, against its nine steps called one by one, byte for
byte; behind it every merged point is re-triangulated from views of BOTH groups, which the sequence without the map update cannot do.
Scene 3 of tests/golden/mergeconstraints_golden.npz, as tests/test_mergeconstraints_solve_gpu.py::test_info_buffers_feed_merge_apply uses it:
it has an older key frame to hold fixed."""
import numpy as np
import pytest

import coslam_amd
from tests import mergeapply_ref as aref
from tests import mergeconstraints_ref as ref
from tests import mergemap_ref as mref
from tests.mergeapply_golden_util import inv_k
from tests.mergeconstraints_golden_util import load
from tests.mergemap_dev import SIGMA, TABLES, Live

pytestmark = pytest.mark.gpu

SCENES = load()


def _step_by_step(L, with_map=True):
    """the nine steps of MergeCamGroups.run called one by one -> (views, pointMap, solved points, recompute counts, apply counts, groups)"""
    import torch

    S, D, T = L.S, L.D, L.tables
    frames = [int(f) for f in S["key_frames"]]
    k, _order = coslam_amd.merge_first_constrain(frames, S["self_motion"], L.ids)                                          # 1
    mc = coslam_amd.MergeConstraints(S["nC"], S["N"], len(S["matches"]), S["nMap"])
    mc.assemble(D.th, D.cams, T["featRef"], S["nMap"], T["mapPts"], D.groups.data_ptr(), *L.pair, frames[k], frames[-1], S["matches"])   # 2
    mc.solve()                                                                                                            # 3
    mc.info_solved(D.groups.data_ptr(), S["gId1"], S["gId2"])                                                             # 4
    ints, _R, _t = mc.infos()
    views, pm, pts = mc.views().tolist(), mc.problem()["pointMap"], mc.solution(1)["pts"]
    cnt = torch.zeros(10, dtype=torch.int32, device=L.dev)
    if with_map:
        mc.apply_map([c["slot2map"] for c in L.cams], T["pointFeat"], T["featRef"], T["refStatic"], S["nMap"], T["mapPts"], True, cnt.data_ptr())   # 5
    plan = coslam_amd.merge_keygraph_plan(frames, L.key_groups, L.ids, k, S["maxiCam"], S["maxjCam"], ints[:, [0, 1, 3, 4]])   # 6
    ma = coslam_amd.MergeApply(plan, frames, S["nC"])
    ma.run_dev(D.th, mc.buf.infoR, mc.buf.infoT)                                                                          # 7
    ma.recompute(D.th, L.cams, T["featRef"], S["nMap"], None, T["firstFrame"], T["lastFrame"], T["mapFlags"], T["mapPts"], T["mapCov"],
                 int(ma.key_frames[0]), SIGMA, True, cnt[6:].data_ptr())                                                  # 8
    ma.status()
    valid = ints[ints[:, 2] >= 0]
    got = coslam_amd.merge_matched_groups(S["groups"], valid[:, 2], valid[:, 5], S["maxiCam"], S["maxjCam"])              # 9
    c = cnt.cpu().tolist()
    ma.close()
    mc.close()
    return dict(views=views, pointMap=pm, pts=pts, apply_counts=c[:6], recompute_counts=c[6:], groups=got)


def _restated_recompute(L, st, feat_ref, M0):
    """tests/mergeapply_ref.py's recomputeMapPoints over the device's corrected poses -> (M, cov, counts, detail)"""
    S, D = L.S, L.D
    pool = np.ascontiguousarray(np.asarray(S["segPool"], np.int32)[:, :max(D.n_seg, 1)])
    iK = np.stack([inv_k(k) for k in np.asarray(S["K"], np.float64)])
    M, cov, det = np.array(M0, np.float64), np.zeros((S["nMap"], 9)), {}
    f2 = S["frame0"] + S["nF"] - 1
    cnt = aref.recompute_map_points_keyfrms(np.asarray(S["K"], np.float64), iK, st["histR"], st["histT"], np.asarray(S["histXY"], np.float64),
                                            S["frame0"], np.asarray(feat_ref, np.int32), pool, None, np.full(S["nMap"], S["frame0"]),
                                            np.full(S["nMap"], f2), np.zeros(S["nMap"], np.uint8), int(S["key_frames"][0]), f2,
                                            S["key_frames"], M, cov, SIGMA, detail=det)
    return M, cov, cnt, det


def test_run_equals_its_steps_and_triangulates_across_both_groups(hip):
    S, G = SCENES[3]
    g1, g2 = set(S["groups"][S["gId1"]]), set(S["groups"][S["gId2"]])
    # ---- the one call
    A = Live(S)
    mg = coslam_amd.MergeCamGroups(S["nC"], S["N"], len(S["matches"]), S["nMap"])
    rep = A.run(mg)
    a = A.state()
    assert rep["status"] == "merged" and rep["merged"] and rep["verdict"] == 1 and mg.last_merge_frame == int(S["key_frames"][-1])
    assert rep["header"]["nMergedTracks"] == len(S["matches"]) and rep["solver"][1].cost >= 0
    # ---- its steps one by one, on a scene of their own
    B = Live(S)
    steps = _step_by_step(B)
    b = B.state()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert rep["apply_counts"] == steps["apply_counts"] and rep["recompute_counts"] == steps["recompute_counts"]
    assert rep["groups"] == steps["groups"]["groups"] and [sorted(g) for g in rep["groups"]] == [sorted(g1 | g2)]
    assert list(rep["group_id"]) == list(steps["groups"]["group_id"]) and rep["merged_gid"] == steps["groups"]["merged_gid"]
    assert bytes(rep["record"]) == bytes(steps["groups"]["record"])
    # ---- the restatement: tables from the list, the points from the re-triangulation over the device's corrected poses
    want = mref.apply_map(A.S, steps["views"], steps["pointMap"], steps["pts"])
    for k in ("slot2map", "featRef", "refStatic", "pointFeat"):
        assert a[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), k
    assert rep["apply_counts"] == want["counts"]
    M, cov, cnt, det = _restated_recompute(A, a, want["featRef"], want["M"])
    assert rep["recompute_counts"] == cnt and a["M"].tobytes() == M.tobytes() and a["cov"].tobytes() == cov.tobytes()
    merged = sorted(set(v[3] for v in steps["views"]))
    assert merged
    for m in merged:
        cams = set(c for c, _, _ in det[m]["views"])
        assert cams & g1 and cams & g2, (m, cams)
    assert a["histR"].tobytes() != np.asarray(S["histR"], np.float64).tobytes()                  # a real correction
    assert not np.array_equal(a["M"][merged], np.asarray(S["M"], np.float64)[merged])
    # ---- the sequence as it stood without the map update: the same rows only get views from one group
    C = Live(S)
    _step_by_step(C, with_map=False)
    c = C.state()
    for k in ("slot2map", "featRef", "refStatic", "pointFeat"):
        assert c[k].tobytes() == np.ascontiguousarray(mref.tables(C.S)[k]).tobytes(), k
    M0, cov0, cnt0, det0 = _restated_recompute(C, c, C.S["featRef"], C.S["M"])
    assert c["M"].tobytes() == M0.tobytes() and c["cov"].tobytes() == cov0.tobytes()
    for m in merged:
        cams = set(cc for cc, _, _ in det0[m]["views"])
        assert cams and not (cams & g1 and cams & g2), (m, cams)
    assert c["histR"].tobytes() == a["histR"].tobytes() and c["M"].tobytes() != a["M"].tobytes()
    # ---- a second run inside the hold-off is refused and enqueues nothing
    again = A.run(mg)
    assert again["status"] == "held_off" and not again["merged"]
    a2 = A.state()
    for k in a:
        assert a[k].tobytes() == a2[k].tobytes(), k
    mg.close()
    for x in (A, B, C):
        x.close()


def test_rejected_scene_changes_nothing_and_does_not_arm_the_hold_off(hip):
    S, G = SCENES[2]
    assert int(G["verdict"]) == 0
    A = Live(S)
    before = A.state()
    mg = coslam_amd.MergeCamGroups(S["nC"], S["N"], len(S["matches"]), S["nMap"], last_merge_frame=-1000)
    rep = A.run(mg)
    after = A.state()
    assert rep["status"] == "rejected" and not rep["merged"] and rep["verdict"] == 0 and rep["header"]["avgErr"] == float(G["avgErr"])
    assert rep["apply_counts"] == [0] * 6 and rep["recompute_counts"] == [0] * 4 and rep["groups"] is None
    assert mg.last_merge_frame == -1000
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    for k in TABLES:
        if k in after:
            assert after[k].tobytes() == np.ascontiguousarray(mref.tables(A.S)[k]).tobytes(), k
    mg.close()
    A.close()
