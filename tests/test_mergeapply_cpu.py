"""The merge's map and group side without a device: the restatement (tests/mergeapply_ref.py) against the reference's own
updateStaticPointPositionAtKeyFrms (tests/golden/mergeapply_golden.npz), what the golden file has to hold, cs_merge_matched_groups (host
code of the library) against the restatement, struct and symbol presence, and the end-to-end scene on the host."""
import os

import numpy as np
import pytest

import coslam_amd
from tests import mergeapply_e2e as e2e
from tests import mergeapply_planted as planted
from tests import mergeapply_ref as ref
from tests.mergeapply_dev import recompute_ref
from tests.mergeapply_golden_util import GOLDEN, chain_nodes, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


@pytest.fixture(scope="module")
def scenes():
    g = np.load(GOLDEN)
    return [scene(g, sc) for sc in range(int(g["n_scenes"]))]


def test_restatement_reproduces_the_reference_bit_for_bit(scenes):
    assert os.path.getsize(GOLDEN) < 300 * 1024
    assert [S["nC"] for S in scenes] == [3, 4, 6, 12] and all(80 <= S["nF"] <= 160 for S in scenes)
    for sc, S in enumerate(scenes):
        gaps = np.diff(S["key_frames"])
        assert gaps.min() >= 3 and gaps.max() <= 9 and len(set(gaps.tolist())) > 3 and S["key_frames"][-1] == S["frame0"] + S["nF"] - 1
        M, cov, cnt = recompute_ref(S, ref)
        moved = (S["M_ref"] != S["M0"]).any(axis=1)
        assert np.array_equal(M, S["M_ref"]) and np.array_equal(cov, S["cov_ref"]), sc
        assert cnt[0] == int(S["selected"].sum()) and cnt[1] == int(moved.sum()) and cnt[1] + cnt[2] == cnt[0] and cnt[3] == 0
        sel = (S["flags"] == 0) & (S["lastFrame"] >= S["f_start"]) & (S["firstFrame"] <= S["f_end"])
        assert np.array_equal(sel, S["selected"].astype(bool))
        # the literal form -- angles through acos, strict > from 0 -- chooses the same views
        M2, cov2 = S["M0"].copy(), S["cov0"].copy()
        ref.recompute_map_points_keyfrms(S["K"], S["iK"], S["histR"], S["histT"], S["histXY"], S["frame0"], S["featRef"], S["segPool"], None,
                                         S["firstFrame"], S["lastFrame"], S["flags"], S["f_start"], S["f_end"], S["key_frames"], M2, cov2,
                                         S["sigma"], angles=True)
        assert np.array_equal(M2, S["M_ref"])


def test_golden_file_holds_what_it_has_to(scenes):
    """the generator's counts, re-asserted from the file: at least 30 of each over the four scenes"""
    tot = dict(head_not_key=0, only_head=0, filter_changes=0, behind_gap=0, few_views=0, before=0, after=0, flag1=0, flag2=0, flag4=0, standing=0,
               rotating=0, filter_points=0)
    for S in scenes:
        keys, frame0, cur = [int(k) for k in S["key_frames"]], S["frame0"], S["frame0"] + S["nF"] - 1
        keyset, all_frames = set(keys), list(range(frame0, cur + 1))
        det = {}
        cnt = recompute_ref(S, ref, detail=det)[2]
        tot["few_views"] += cnt[2]
        tot["before"] += int((S["lastFrame"] < S["f_start"]).sum())
        tot["after"] += int((S["firstFrame"] > S["f_end"]).sum())
        for b in (1, 2, 4):
            tot[f"flag{b}"] += int((S["flags"] == b).sum())
        tot["filter_points"] += len(S["filter_points"])
        Rl, Tl = S["histR"].tolist(), S["histT"].tolist()
        centre = lambda c, f: ref.cam_center(Rl[c][f - frame0], Tl[c][f - frame0])  # noqa: E731
        for m, rec in det.items():
            M0 = [float(v) for v in S["M0"][m]]
            for c in range(S["nC"]):
                r4 = S["featRef"][m, c]
                if r4[0] < 0:
                    continue
                if int(r4[1]) not in keyset:
                    tot["head_not_key"] += any(f in keyset for f, _ in chain_nodes(r4, S["segPool"][c])[1:])
                    assert c not in rec["walks"]
                    continue
                w = rec["walks"][c]
                if not w["nodes"]:
                    tot["only_head"] += 1
                elif w["node"] is None:
                    tot["rotating"] += 1
                else:
                    best = min(v for _, _, v in w["nodes"])
                    ties = [f for f, _, v in w["nodes"] if v == best]
                    tot["standing"] += len(ties) > 1
                    assert w["node"][1] == max(ties)                                  # the newest of equals
                    tot["behind_gap"] += w["node"][0] != int(r4[0])
                    wa = ref.walk_widest_key_node(c, r4, S["segPool"], S["segPool"].shape[1], S["N"], all_frames, frame0, cur, centre, M0,
                                                  centre(c, int(r4[1])))
                    tot["filter_changes"] += wa["node"][1] not in keyset
    print(tot)
    assert all(v >= 30 for v in tot.values()), tot


def test_planted_scenes_take_the_planted_views():
    S, want = planted.block_edges()
    det = {}
    assert recompute_ref(S, ref, detail=det)[2] == [4, 4, 0, 0]
    assert all(det[p]["walks"][c]["node"][1] == want[p][c] for p in range(4) for c in range(len(planted.RUNS)))
    S, want = planted.equal_maxima()
    det = {}
    recompute_ref(S, ref, detail=det)
    assert [det[0]["walks"][c]["node"][1] for c in range(3)] == want[0]


CASES = [
    ("two groups", [[0, 1], [2]], [(0, 1)], 0, 2),
    ("chain 0-1, 1-2", [[0], [1, 3], [2], [4]], [(0, 1), (1, 2)], 0, 2),
    ("two separate merges", [[0], [1], [2], [3], [4]], [(0, 3), (1, 4)], 1, 4),
    ("infos given as (2, 0)", [[0], [1], [2]], [(2, 0)], 2, 0),
    ("a group order [0, 2, 1]", [[0, 2, 1], [3, 5], [4]], [(1, 0)], 5, 0),
    ("16 singleton groups", [[c] for c in range(16)], [(15, 0), (3, 7), (7, 9)], 9, 3),
    ("mergedGid is not group 0", [[0], [1], [2]], [(1, 2)], 2, 1),
]


@pytest.mark.parametrize("name,groups,infos,cam1,cam2", CASES, ids=[c[0] for c in CASES])
def test_merge_matched_groups_against_the_restatement(name, groups, infos, cam1, cam2):
    g1, g2 = [a for a, _ in infos], [b for _, b in infos]
    got = coslam_amd.merge_matched_groups(groups, g1, g2, cam1, cam2)
    want = ref.merge_matched_groups(groups, g1, g2, cam1, cam2)
    assert got["groups"] == want[0] and [int(v) for v in got["group_id"]] == want[1] and got["merged_gid"] == want[2]
    rec = got["record"]
    assert rec.groupNum == len(want[0]) and all(rec.num[g] == 0 for g in range(rec.groupNum, 16))
    assert all(rec.camIds[g][i] == -1 for g in range(16) for i in range(rec.num[g], 16))
    assert sorted(c for g in got["groups"] for c in g) == sorted(c for g in groups for c in g)


def test_merge_matched_groups_expected_records():
    assert coslam_amd.merge_matched_groups([[0], [1, 3], [2], [4]], [0, 1], [1, 2], 0, 2)["groups"] == [[0, 1, 3, 2], [4]]
    assert coslam_amd.merge_matched_groups([[0], [1], [2], [3], [4]], [0, 1], [3, 4], 1, 4)["groups"] == [[0, 3], [1, 4], [2]]
    assert coslam_amd.merge_matched_groups([[0, 2, 1], [3, 5], [4]], [1], [0], 5, 0)["groups"] == [[0, 2, 1, 3, 5], [4]]


def test_merge_matched_groups_refuses_where_the_reference_asserts():
    with pytest.raises(coslam_amd.CoslamHipError) as ei:
        coslam_amd.merge_matched_groups([[0, 1], [2]], [0], [1], 5, 6)               # camid1 / camid2 in no group
    assert f"code {INVALID}" in str(ei.value) and "camera 5" in str(ei.value)
    assert ref.merge_matched_groups([[0, 1], [2]], [0], [1], 5, 6) is None
    with pytest.raises(coslam_amd.CoslamHipError, match="names group"):
        coslam_amd.merge_matched_groups([[0, 1], [2]], [0], [2], 0, 2)


def test_symbols_and_structs():
    L = coslam_amd.lib()
    for name in ("cs_recompute_map_points_keyfrms_dev", "cs_merge_apply_create", "cs_merge_apply_run_dev", "cs_merge_apply_status",
                 "cs_merge_apply_guard", "cs_merge_apply_destroy", "cs_merge_matched_groups", "cs_track_history_set_span_guarded_dev"):
        assert hasattr(L, name), name
    hdr = open(os.path.join(ROOT, "include", "coslam_hip.h")).read()
    for name in ("cs_recompute_map_points_keyfrms_dev", "cs_merge_apply_run_dev", "cs_merge_matched_groups", "cs_track_history_set_span_guarded_dev"):
        assert name + "(" in hdr
    assert all(hasattr(coslam_amd, n) for n in ("MergeApply", "merge_matched_groups", "recompute_map_points_keyfrms_dev", "MergePoseCorrection"))


def test_end_to_end_scene_on_the_host():
    """the whole sequence with the restatements only: the drifted group's own points, seen from the other group's cameras at the current key
    frame, land nearer to where those cameras see them once poses and points are corrected (the figures are DESIGN 3.21's)"""
    E = e2e.build()
    S = E["S"]
    assert S["nC"] == 4 and S["N"] == 64 and len(S["X"]) == 192 and len(S["key_frames"]) == 6 and S["nF"] == 21
    M0, cov0 = e2e.start_points(E, ref)
    hR, hT = e2e.corrected_poses_host(E)
    M, cov = M0.copy(), cov0.copy()
    cnt = ref.recompute_map_points_keyfrms(S["K"], S["iK"], hR, hT, S["histXY"], S["frame0"], S["featRef"], S["segPool"], None, S["firstFrame"],
                                           S["lastFrame"], S["flags"], S["f_start"], S["f_end"], S["key_frames"], M, cov, S["sigma"])
    before, after = e2e.reproj_median(E, M0, S["histR"], S["histT"]), e2e.reproj_median(E, M, hR, hT)
    print(f"median reprojection error: before {before:.3f} px, after {after:.3f} px; counts {cnt}")
    assert cnt == [192, 192, 0, 0] and after < before
    groups, gid, mg = ref.merge_matched_groups(E["groups"], [0], [1], E["m"]["camid1"], E["m"]["camid2"])
    assert groups == [[0, 1, 2, 3]] and gid[:4] == [0, 0, 0, 0] and mg == 0
