"""Writes tests/golden/mergeconstraints_golden.npz: the reference's OWN MergeCameraGroup::genMergeInfoVer2 (with a solver stand-in that records
its arguments and changes nothing) on six scenes built with its classes -- the fixture of cs_merge_first_constrain,
cs_merge_constraints_assemble_dev and cs_merge_info_dev.  Needs oracle/_ref/ref_mergeconstraints_test
(tests/cxx/ref_mergeconstraints_test.cpp, built by oracle/Makefile); where the reference tree exists:

    python tests/golden/make_golden.py mergeconstraints

Every case the fixture has to hold is ASSERTED below (COVER), counted with the restatement tests/mergeconstraints_ref.py after it has been
checked against the reference's output, so a scene cannot silently stop covering its case.  The file holds data only."""
import os
import struct
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import mergeconstraints_ref as ref  # noqa: E402
from tests.golden.fixtures import run_driver  # noqa: E402
from tests.mergeconstraints_golden_util import RESULT_KEYS, SCENE_KEYS, expand  # noqa: E402
from tests.mergeconstraints_scenes import make_scene, write_input  # noqa: E402

SEED = 22

# groups (discovery order, not ascending), the two groups, maxiCam / maxjCam, frames held, key-frame gaps back from the current frame,
# self-motion per older key frame (newest first) as the set of cameras that moved, points per side, matches, what the matches plant
SPECS = [
    dict(groups=[[0, 1], [2]], g=(0, 1), ij=(1, 2), nF=14, gaps=(3, 4, 5), moved=[{0, 2}, {0, 1, 2}, {1}], nA=40, nB=25, nMatch=8, plant="mixed"),
    dict(groups=[[0, 2, 1, 4, 3], [6, 5, 8, 7], [9]], g=(0, 1), ij=(2, 6), nF=12, gaps=(2, 3, 4), moved=[{0, 5}, set(), {0, 1, 2, 3, 4, 5, 6, 7, 8}],
         nA=45, nB=40, nMatch=10, plant="mixed"),
    dict(groups=[[0, 1], [2, 3]], g=(1, 0), ij=(3, 0), nF=10, gaps=(2, 3, 2), moved=[{2}, set(), set()], nA=20, nB=20, nMatch=6, plant="reject"),
    dict(groups=[[0, 1], [3, 2]], g=(0, 1), ij=(0, 2), nF=10, gaps=(3, 2, 2), moved=[{0, 1, 2, 3}, {1}, set()], nA=45, nB=45, nMatch=3, plant="clean"),
    dict(groups=[[1], [0], [2, 3]], g=(0, 2), ij=(1, 3), nF=16, gaps=(5, 5, 4), moved=[{1}, {2, 3}, {1, 2, 3}], nA=25, nB=30, nMatch=7, plant="mixed"),
    dict(groups=[[0, 1, 2], [3, 4, 5, 6]], g=(1, 0), ij=(4, 1), nF=12, gaps=(3, 3, 3), moved=[{0, 1, 2, 3, 4, 5, 6}, {3}, {0}], nA=35, nB=35, nMatch=12,
         plant="shared"),
]
COVER = ("groups_2_1", "nine_cameras", "reject", "cap_binds", "listed_three_times", "duplicate_view", "f1_through_segment", "gap_over_f1",
         "one_view_track", "unmapped_match")


class Reader:
    def __init__(self, raw):
        self.raw, self.off = raw, 0

    def ints(self, n):
        v = np.frombuffer(self.raw, "<i4", n, self.off).copy()
        self.off += 4 * n
        return v

    def i(self):
        return int(self.ints(1)[0])

    def dbl(self, n):
        v = np.frombuffer(self.raw, "<f8", n, self.off).copy()
        self.off += 8 * n
        return v


def read_output(rd, S):
    nC, N, nMap = S["nC"], S["N"], S["nMap"]
    G = dict(verdict=np.int32(rd.i()), avgErr=np.float64(rd.dbl(1)[0]), first_frame=np.int32(rd.i()))
    n_pose = rd.i()
    G["order"] = rd.ints(2 * n_pose).reshape(-1, 2).astype(np.int16)
    calls = rd.i()
    z = np.zeros
    G.update(ba_args=z((0, 5)), Ks=z((0, 9)), Rs=z((0, 9)), Ts=z((0, 3)), pts=z((0, 3)), pointMap=z(0, np.int16), obs_ptr=z(1, np.int32),
             obs_cam=z(0, np.int16), obs_xy=z((0, 2)))
    if calls:
        assert calls == 2
        args = []
        for _ in range(2):
            a = rd.ints(4)
            args.append([float(v) for v in a] + [float(rd.dbl(1)[0])])
        C, P, n_obs = rd.ints(3)
        G.update(ba_args=np.array(args), Ks=rd.dbl(9 * C).reshape(C, 9), Rs=rd.dbl(9 * C).reshape(C, 9), Ts=rd.dbl(3 * C).reshape(C, 3),
                 pts=rd.dbl(3 * P).reshape(P, 3), pointMap=rd.ints(P).astype(np.int16), obs_ptr=rd.ints(P + 1), obs_cam=rd.ints(n_obs).astype(np.int16),
                 obs_xy=rd.dbl(2 * n_obs).reshape(n_obs, 2))
    n_info = rd.i()
    ints, E, R, t = [], [], [], []
    for _ in range(n_info):
        ints.append(rd.ints(7))
        E.append(rd.dbl(9)), R.append(rd.dbl(9)), t.append(rd.dbl(3))
    G.update(info_ints=np.array(ints, np.int16).reshape(-1, 7), info_E=np.array(E).reshape(-1, 9), info_R=np.array(R).reshape(-1, 9),
             info_t=np.array(t).reshape(-1, 3))
    G["cur_mpt"] = rd.ints(nC * N).reshape(nC, N).astype(np.int16)
    G["pfeat"] = rd.ints(nMap * nC * 2).reshape(nMap, nC, 2).astype(np.int16)
    n_det = rd.i()
    G["detached"] = rd.ints(3 * n_det).reshape(-1, 3).astype(np.int16)
    return G


def check_and_cover(S, G, cover):
    """the restatement reproduces the reference bit for bit; what the scene covers"""
    fc = ref.first_constrain(S["key_frames"], S["self_motion"], ref.cam_ids_in_both_groups(S["groups"], S["gId1"], S["gId2"]))
    assert int(S["key_frames"][fc[0]]) == int(G["first_frame"]) and fc[1] == [tuple(int(v) for v in r) for r in G["order"]]
    det = {}
    A = ref.assemble(S, int(G["first_frame"]), detail=det)
    assert A["verdict"] == int(G["verdict"]) and A["avgErr"] == float(G["avgErr"]), (A["verdict"], A["avgErr"], G["verdict"], G["avgErr"])
    cur, pfeat, detached = ref.apply_views(S, A["views"], int(G["first_frame"]))
    assert np.array_equal(np.array(cur), G["cur_mpt"]) and np.array_equal(np.array(pfeat), G["pfeat"])
    assert [list(d) for d in detached] == sorted(G["detached"].tolist())
    sizes = sorted(len(g) for g in (S["groups"][S["gId1"]], S["groups"][S["gId2"]]))
    cover["groups_2_1"] += sizes == [1, 2]
    cover["nine_cameras"] += sum(sizes) >= 9
    cover["unmapped_match"] += A["skipped"] > 0
    if A["verdict"] != ref.VERDICT_MERGE:
        assert len(G["info_ints"]) == 0 and len(G["pts"]) == 0
        cover["reject"] += 1
        return A
    for k in ("Ks", "Rs", "Ts", "pts", "obs_xy"):
        assert np.array_equal(np.array(A[k]).reshape(G[k].shape), G[k]), k
    for k in ("pointMap", "obs_ptr", "obs_cam"):
        assert np.array_equal(np.array(A[k]), G[k]), k
    ints, R, t = ref.merge_infos(S, A["Rs"], A["Ts"], A["order"])
    assert np.array_equal(np.array(ints), G["info_ints"][:, :6]) and (G["info_ints"][:, 6] == 1).all()
    assert np.array_equal(np.array(R), G["info_R"]) and np.array_equal(np.array(t), G["info_t"])
    assert G["ba_args"].tolist() == [[1, 1, 1, 100, 800], [1, 1, 5, 30, 30]]
    nT = A["nMergedTracks"]
    qualifying = sum(1 for q in det["cand"] if any(ref_cur(S, q, c) for c in A["cam_ids"]))
    cover["cap_binds"] += len(S["matches"]) == 3 and det["n_candidates"] > 60 and qualifying > 20 * nT == A["nUnmerged"]
    counts = {}
    for q in det["cand"]:
        counts[q] = counts.get(q, 0) + 1
    pm = A["pointMap"]
    cover["listed_three_times"] += any(n >= 3 and pm.count(q) >= 3 for q, n in counts.items())
    cover["duplicate_view"] += any(v[5] & ref.VIEW_DETACHED for v in A["views"])
    cover["one_view_track"] += det["dropped_tracks"] > 0
    f1, f2 = int(G["first_frame"]), S["frame0"] + S["nF"] - 1
    for (m, tk), pv in zip(det["tracks"], det["prev"]):
        for (c, s, _, first, seg), ps in zip(tk, pv):
            if first > f1 and ps >= 0:
                cover["f1_through_segment"] += 1
            if first > f1 and seg >= 0 and ps < 0:
                older = [int(v) for v in S["segPool"][c][seg]]
                while older[1] > f1 and older[3] >= 0:
                    older = [int(v) for v in S["segPool"][c][older[3]]]
                cover["gap_over_f1"] += older[1] < f1
    return A


def ref_cur(S, m, c):
    r = S["featRef"][m][c]
    return int(r[0]) >= 0 and int(r[1]) == S["frame0"] + S["nF"] - 1


def mergeconstraints_case():
    rng = np.random.default_rng(SEED)
    raws = [make_scene(sc, spec, rng) for sc, spec in enumerate(SPECS)]
    scenes = [expand(r) for r in raws]
    with tempfile.TemporaryDirectory() as td:
        pin, pout = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(pin, "wb") as f:
            f.write(struct.pack("i", len(scenes)))
            for S in scenes:
                write_input(f, S)
        print(run_driver("ref_mergeconstraints_test", "golden", pin, pout).strip())
        rd = Reader(open(pout, "rb").read())
    out = dict(n_scenes=np.int32(len(scenes)), seed=np.int32(SEED))
    cover = {k: 0 for k in COVER}
    for sc, (raw, S) in enumerate(zip(raws, scenes)):
        G = read_output(rd, S)
        A = check_and_cover(S, G, cover)
        print(f"scene {sc}: {S['nC']} cameras, N {S['N']}, {S['nMap']} points, verdict {A['verdict']}, avgErr {A['avgErr']:.4f}, "
              f"{A['nMergedTracks']} merged + {A['nUnmerged']} unmerged tracks, {A['nPrevViews']} views in the first-constrained frame, "
              f"{len(A['pointMap'])} points, {len(A['obs_cam'])} measurements, {A['skipped']} matches skipped")
        for k in SCENE_KEYS:
            out[f"s{sc}_{k}"] = raw[k]
        for k in RESULT_KEYS:
            out[f"s{sc}_{k}"] = G[k]
    assert rd.off == len(rd.raw)
    print("covered:", cover)
    for k, v in cover.items():
        assert v > 0, f"no scene covers {k}"
    return out
