"""Loader of tests/golden/mergematch_golden.npz (written by tests/golden/make_mergematch_golden.py): the scenes in the layout of
tests/mergematch_scenes.py and what the reference's own storeFeaturePoints / matchFeaturePointsNCC / matchMergableCameras gave on them."""
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mergematch_golden.npz")


def load():
    """-> [(S, G)]: S = dict(nC, N, Ws, Hs, frame, scale, par, groups, cams, entries); G = dict(ran, F, matches (SLOT pairs in the
    reference's order), scores, loop = [numMatched, called, maxgId1, maxgId2, maxiCam, maxjCam, m_gid1, m_gid2, m_camid1, m_camid2],
    rec_matches = the Matching handed to genMergeInfoVer2)"""
    z = np.load(PATH)
    out = []
    for k in range(int(z["n_scenes"])):
        p = "s%d_" % k
        nC, N, Ws, Hs, frame, nE = (int(v) for v in z[p + "dims"])
        par = z[p + "par"]
        cams = [dict(K=z[p + "K"][c], xy=z[p + "xy"][c], state=z[p + "state"][c], imgSmall=z[p + "img"][c], imgScale=float(par[0])) for c in range(nC)]
        S = dict(nC=nC, N=N, Ws=Ws, Hs=Hs, frame=frame, scale=float(par[0]), par=tuple(float(v) for v in par[1:]),
                 groups=[[int(c) for c in g if c >= 0] for g in z[p + "groups"]], cams=cams, entries=[])
        G = dict(ran=[], F=[], matches=[], scores=[], loop=z[p + "loop"], rec_matches=z[p + "rec_matches"].reshape(-1, 2))
        for e in range(nE):
            q = "%se%d_" % (p, e)
            ids = z[q + "ids"]
            S["entries"].append(dict(iCam=int(ids[0]), gId1=int(ids[1]), jCam=int(ids[2]), gId2=int(ids[3]), surf1=z[q + "surf1"], surf2=z[q + "surf2"],
                                     idx=z[q + "idx"], E=z[q + "E"], flags=z[q + "flags"]))
            G["ran"].append(int(ids[4])), G["F"].append(z[q + "F"]), G["matches"].append(z[q + "matches"].reshape(-1, 2)), G["scores"].append(z[q + "scores"])
        out.append((S, G))
    return out


def front(S, G):
    """what the host front hands the selection: infos (frame, cam1, gid1, frame, cam2, gid2), SURF match counts, computeEMat > 0, NCC counts"""
    infos = [(S["frame"], q["iCam"], q["gId1"], S["frame"], q["jCam"], q["gId2"]) for q in S["entries"]]
    surf = [len(q["idx"]) for q in S["entries"]]
    ok = [1 if int(q["flags"].sum()) >= 15 else 0 for q in S["entries"]]
    return infos, surf, ok, [len(m) for m in G["matches"]]
