#!/usr/bin/env python
"""Writes tests/golden/mergematch_golden.npz: the scenes of tests/mergematch_scenes.py with what the reference's OWN
MergeCameraGroup::storeFeaturePoints / matchFeaturePointsNCC / matchMergableCameras give on them (oracle/_ref/ref_mergematch_test, built
by oracle/Makefile where the reference tree exists).  Run from the repository's root:
    python tests/golden/make_golden.py mergematch
Scene 2 is scene 1 again with the driver's own calls at nccMin = the score of one of its candidates (found with the restatement; the
reference then decides what a candidate exactly at nccMin does).  COVER lists the cases the fixture must hold; each is asserted here."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import mergematch_ref as R           # noqa: E402
from tests.golden.fixtures import run_driver    # noqa: E402
from tests import mergematch_scenes as MS       # noqa: E402

COVER = ["two group pairs, three matched entries, the i != k quirk changes the winner", "an entry with fewer than 25 SURF matches",
         "an entry whose computeEMat fails", "both orientations of m_gid1 / m_gid2", "features within 5 px of the small image's border",
         "dead slots between live ones", "two seeds equidistant from a feature", "a candidate exactly at maxDisp", "a candidate exactly at epiMax",
         "a candidate exactly at nccMin", "bit-equal scores competing for a row", "bit-equal scores competing for a column"]


def flatten(k, S, G):
    out = {}
    p = "s%d_" % k
    out[p + "dims"] = np.array([S["nC"], S["N"], S["Ws"], S["Hs"], S["frame"], len(S["entries"])], np.int32)
    out[p + "par"] = np.array([S["scale"], *S["par"]], np.float64)
    out[p + "groups"] = np.array([[g[i] if i < len(g) else -1 for i in range(16)] for g in S["groups"]], np.int32)
    out[p + "K"] = np.stack([c["K"] for c in S["cams"]])
    out[p + "xy"] = np.stack([c["xy"] for c in S["cams"]])
    out[p + "state"] = np.stack([c["state"] for c in S["cams"]])
    out[p + "img"] = np.stack([c["imgSmall"] for c in S["cams"]])
    for e, q in enumerate(S["entries"]):
        out[p + "e%d_ids" % e] = np.array([q["iCam"], q["gId1"], q["jCam"], q["gId2"], G["ran"][e]], np.int32)
        for n in ("surf1", "surf2", "idx", "E", "flags"):
            out[p + "e%d_%s" % (e, n)] = np.asarray(q[n])
        out[p + "e%d_F" % e], out[p + "e%d_matches" % e], out[p + "e%d_scores" % e] = G["F"][e], G["matches"][e], G["scores"][e]
    out[p + "loop"], out[p + "rec_matches"] = G["loop"], G["rec_matches"]
    return out


def mergematch_case():
    s1 = MS.scene_edges()
    (e, job), = MS.jobs_of(s1)
    ref = R.match_job(s1["cams"], MS.WS, MS.HS, job, *s1["par"])
    mid = sorted(c[3] for c in ref["cands"] if c[3] < 0.98)
    assert len(mid) >= 3, mid
    ncc_min = mid[len(mid) // 2]
    scenes = [MS.scene_quirk(), s1, MS.scene_edges(ncc_min=ncc_min)]
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "in.bin"), "wb") as f:
            MS.write_input(f, scenes)
        print(run_driver("ref_mergematch_test", "golden", os.path.join(d, "in.bin"), os.path.join(d, "out.bin")))
        G = MS.read_output(open(os.path.join(d, "out.bin"), "rb").read(), scenes)
    covered = set()
    # ---- scene 0: the loop's quirk, the skips, the else orientation
    S, g = scenes[0], G[0]
    n = [len(m) for m in g["matches"]]
    assert g["ran"] == [0, 1, 0, 1, 1] and n[3] > n[4] > 20 >= n[1] > 0, (g["ran"], n)
    assert list(g["loop"][:6]) == [1, 1, 0, 1, 1, 2], g["loop"]               # numMatched, called, gId 0 / 1, cameras (1, 2): the entry with FEWER matches
    assert np.array_equal(g["rec_matches"], g["matches"][4])
    covered |= {COVER[0]}
    assert len(S["entries"][2]["idx"]) < 25 and g["ran"][2] == 0
    covered |= {COVER[1]}
    assert len(S["entries"][0]["idx"]) >= 25 and 0 < S["entries"][0]["flags"].sum() < 15 and g["ran"][0] == 0
    covered |= {COVER[2]}
    assert list(g["loop"][6:]) == [1, 0, 2, 1] and list(G[1]["loop"][6:]) == [0, 1, 0, 2], (g["loop"], G[1]["loop"])
    covered |= {COVER[3]}
    # ---- scene 1: the edges
    S, g, nt = scenes[1], G[1], scenes[1]["notes"]
    m = {tuple(r) for r in g["matches"][0].tolist()}
    xy0, xy2, st0 = S["cams"][0]["xy"], S["cams"][2]["xy"], S["cams"][0]["state"]
    assert any((xy0[0, a] * MS.SCALE < 5 or xy0[1, a] * MS.SCALE < 5 or xy0[0, a] * MS.SCALE > MS.WS - 6 or xy0[1, a] * MS.SCALE > MS.HS - 6) for a, _ in m)
    covered |= {COVER[4]}
    assert any(st0[a] < 0 and st0[a + 1] >= 0 for a in range(S["N"] - 1)) and any(st0[a - 1] < 0 for a, _ in m if a)
    covered |= {COVER[5]}
    a, bs = nt["disp"]
    ref = R.match_job(S["cams"], MS.WS, MS.HS, MS.jobs_of(S)[0][1], *S["par"])
    cand = {(c[0], c[1]): c for c in ref["cands"]}
    # (a, bs[0]) and (a, bs[1]) have bit-equal scores; the guide keeps both only under the FIRST of the two equidistant seeds; the walk takes bs[0]
    assert (a, bs[0]) in m and cand[(a, bs[0])][3] == cand[(a, bs[1])][3]
    kept = {(c[0], c[1]) for c in R.guide(ref["cands"], xy0, xy2, MS.jobs_of(S)[0][1]["seeds"], 150.0)}
    assert (a, bs[1]) in kept and xy2[0, bs[1]] - xy0[0, a] - 12.0 == 150.0
    sd = MS.jobs_of(S)[0][1]["seeds"]
    d2 = (sd[:, 0] - xy0[0, a]) ** 2 + (sd[:, 1] - xy0[1, a]) ** 2
    assert (d2 == d2.min()).sum() == 2
    covered |= {COVER[6], COVER[7]}
    a2, b2 = nt["disp_out"]
    assert (a2, b2[1]) in cand and (a2, b2[1]) not in kept
    # the reference itself: take (a, bs[0]) away and the candidate exactly at maxDisp must be the row's match -- asserted through the device
    # tests on the restated list; here the reference's matches hold the row's winner and none of the pair beyond maxDisp
    assert (a2, b2[0]) in m and (a2, b2[1]) not in m
    a, bs = nt["epi"]
    assert (a, bs[1]) in cand and cand[(a, bs[1])][2] == 20.0 and (a, bs[2]) not in cand
    covered |= {COVER[8]}
    a, bs = nt["row"]
    assert cand[(a, bs[0])][3] == cand[(a, bs[1])][3] and (a, bs[0]) in m and (a, bs[1]) not in m and bs[0] < bs[1]
    covered |= {COVER[10]}
    aa, b = nt["col"]
    assert cand[(aa[0], b)][3] == cand[(aa[1], b)][3] and (aa[0], b) in m and (aa[1], b) not in m and aa[0] < aa[1]
    covered |= {COVER[11]}
    # ---- scene 2: the candidate exactly at nccMin is kept by the reference, the next one below is not
    g2 = G[2]
    at = [(c[0], c[1]) for c in ref["cands"] if c[3] == ncc_min]
    below = [(c[0], c[1]) for c in ref["cands"] if c[3] < ncc_min]
    m2 = {tuple(r) for r in g2["matches"][0].tolist()}
    assert len(at) == 1 and at[0] in m2 and below and not (set(below) & m2) and set(below) & m
    assert ncc_min in g2["scores"][0].tolist()
    covered |= {COVER[9]}
    assert covered == set(COVER), set(COVER) - covered
    out = dict(n_scenes=np.array(len(scenes), np.int32))
    for k, (S, g) in enumerate(zip(scenes, G)):
        out.update(flatten(k, S, g))
    return out
