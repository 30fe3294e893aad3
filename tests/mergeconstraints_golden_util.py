"""tests/golden/mergeconstraints_golden.npz -> the scene dicts tests/mergeconstraints_ref.py takes and the reference's recorded results
(shared by tests/golden/make_mergeconstraints_golden.py, which writes the file, and the tests, which read it).

The file stores poses, intrinsics, map points and pixels as float32 and they are USED as exactly those values in binary64 (the reference's
function takes them as given); integers are stored in the narrowest type that holds them."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mergeconstraints_golden.npz")

SCENE_KEYS = ("frame0", "key_frames", "self_motion", "groups", "gids", "K", "R", "t", "M", "state", "slot2map", "xy", "featRef", "segPool",
              "matches")
RESULT_KEYS = ("verdict", "avgErr", "first_frame", "order", "ba_args", "Ks", "Rs", "Ts", "pts", "pointMap", "obs_ptr", "obs_cam", "obs_xy",
               "info_ints", "info_E", "info_R", "info_t", "cur_mpt", "pfeat", "detached")


def expand(raw):
    """the stored arrays of one scene -> S"""
    K = np.asarray(raw["K"]).astype(np.float64).reshape(-1, 9)
    nC = K.shape[0]
    R = np.asarray(raw["R"]).astype(np.float64).reshape(nC, -1, 9)
    nF = R.shape[1]
    xy = np.asarray(raw["xy"]).astype(np.float64).reshape(nC, nF, -1)
    N = xy.shape[2] // 2
    g = np.asarray(raw["groups"]).astype(np.int32)
    gids = [int(v) for v in raw["gids"]]
    return dict(nC=nC, N=N, nF=nF, frame0=int(raw["frame0"]), key_frames=np.asarray(raw["key_frames"]).astype(np.int32),
                self_motion=np.asarray(raw["self_motion"]).astype(np.int32).reshape(-1, nC), groups=[[int(c) for c in row if c >= 0] for row in g],
                gId1=gids[0], gId2=gids[1], maxiCam=gids[2], maxjCam=gids[3], K=K, histR=R,
                histT=np.asarray(raw["t"]).astype(np.float64).reshape(nC, nF, 3), histXY=xy,
                M=np.asarray(raw["M"]).astype(np.float64).reshape(-1, 3), nMap=int(np.asarray(raw["M"]).reshape(-1, 3).shape[0]),
                state=np.asarray(raw["state"]).astype(np.int32).reshape(nC, N), slot2map=np.asarray(raw["slot2map"]).astype(np.int32).reshape(nC, N),
                featRef=np.asarray(raw["featRef"]).astype(np.int32).reshape(-1, nC, 4),
                segPool=np.asarray(raw["segPool"]).astype(np.int32).reshape(nC, -1, 4), matches=np.asarray(raw["matches"]).astype(np.int32).reshape(-1, 2))


def load():
    """-> [(S, G)] per scene: the scene and the reference's results"""
    g = np.load(GOLDEN)
    out = []
    for sc in range(int(g["n_scenes"])):
        S = expand({k: g[f"s{sc}_{k}"] for k in SCENE_KEYS})
        G = {k: g[f"s{sc}_{k}"] for k in RESULT_KEYS}
        out.append((S, G))
    return out
