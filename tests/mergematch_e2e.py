"""The end-to-end scene of the merge matcher: a merge-constraints scene (tests/mergeconstraints_scenes.py: two camera groups,
a history, a map, planted true correspondences between maxiCam and maxjCam) with small images RENDERED so that true correspondences have
matching patches: every feature of the current key frame carries a windowed sum of six sinusoids of its own, placed at its sub-pixel position
in the small image; the two features of a planted match carry the same one.  E comes from the true poses, the seeds are a subset of the
planted matches."""
import numpy as np

from tests.mergeconstraints_golden_util import expand
from tests.mergeconstraints_scenes import make_scene
from tests.mergemap_dev import with_tables

SPEC = dict(groups=[[0, 1], [3, 2]], g=(0, 1), ij=(0, 2), nF=10, gaps=(3, 2, 2), moved=[{0, 1, 2, 3}, {1}, set()], nA=45, nB=45, nMatch=30,
            plant="clean")
W, H, SCALE = 640, 480, 0.6        # (0.3 would put the blocks of neighbouring features on top of each other in this scene)
WS, HS = 384, 288


def _pattern(rng):
    f = rng.uniform(0.3, 1.2, (6, 2)) * rng.choice([-1.0, 1.0], (6, 2))
    return f, rng.uniform(0, 2 * np.pi, 6)


def render(xy, state, pattern_of_slot, rng):
    """one small image: base 128 with faint noise, plus every live feature's pattern under a Gaussian window of 3 px"""
    img = 128.0 + rng.normal(0, 1.5, (HS, WS))
    N = len(state)
    for s in range(N):
        if state[s] not in (0, 1):
            continue
        fx, fy = xy[s] * SCALE, xy[N + s] * SCALE
        f, ph = pattern_of_slot[s]
        x0, x1, y0, y1 = max(int(fx) - 12, 0), min(int(fx) + 13, WS), max(int(fy) - 12, 0), min(int(fy) + 13, HS)
        if x0 >= x1 or y0 >= y1:
            continue
        yy, xx = np.mgrid[y0:y1, x0:x1].astype(np.float64)
        dx, dy = xx - fx, yy - fy
        w = np.exp(-(dx * dx + dy * dy) / (2 * 3.0 ** 2))
        img[y0:y1, x0:x1] += 22.0 * w * sum(np.cos(f[k, 0] * dx + f[k, 1] * dy + ph[k]) for k in range(6))
    return np.ascontiguousarray(np.clip(np.rint(img), 0, 255).astype(np.uint8))


def essential(Ri, ti, Rj, tj):
    """E of (camera i -> camera j): x_j = R x_i + t, E = [t]x R (formEMat)"""
    Ri, Rj = np.asarray(Ri, np.float64).reshape(3, 3), np.asarray(Rj, np.float64).reshape(3, 3)
    R = Rj @ Ri.T
    t = np.asarray(tj, np.float64) - R @ np.asarray(ti, np.float64)
    X = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return (X @ R).reshape(9)


def build(seed=11, n_seeds=8):
    """-> (S: the expanded scene with tables, cams: mergematch_ref cameras of the current key frame, entry: the gate's entry for the true
    pair, job: dict(E, seeds))"""
    rng = np.random.default_rng(seed)
    S = with_tables(expand(make_scene(3, SPEC, rng)))
    nC, N = S["nC"], S["N"]
    xy = np.asarray(S["histXY"], np.float64)[:, -1]
    state = np.asarray(S["state"], np.int32)
    iC, jC = S["maxiCam"], S["maxjCam"]
    pats = [[_pattern(rng) for _ in range(N)] for _ in range(nC)]
    for a, b in np.asarray(S["matches"]):
        pats[jC][b] = pats[iC][a]
    K = np.asarray(S["K"], np.float64)
    cams = [dict(xy=np.ascontiguousarray(xy[c].reshape(2, N)), state=state[c], K=K[c], imgSmall=render(xy[c], state[c], pats[c], rng), imgScale=SCALE)
            for c in range(nC)]
    R, t = np.asarray(S["histR"], np.float64), np.asarray(S["histT"], np.float64)
    E = essential(R[iC, -1], t[iC, -1], R[jC, -1], t[jC, -1])
    pick = np.asarray(S["matches"])[:: max(1, len(S["matches"]) // n_seeds)][:n_seeds]
    seeds = np.array([[xy[iC][a], xy[iC][N + a], xy[jC][b], xy[jC][N + b]] for a, b in pick])
    f2 = S["frame0"] + S["nF"] - 1
    entry = (f2, iC, S["gId1"], f2, jC, S["gId2"])
    return S, cams, entry, dict(iCam=iC, jCam=jC, E=E, seeds=seeds)
