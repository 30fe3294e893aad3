"""Restatement of MergeCameraGroup::checkPossibleMergable (reference src/app/SL_MergeCameraGroup.cpp:56-177) in numpy / pure Python, branch
by branch with the reference's line numbers, written from the reference's text.  project is numpy f64 in pu_project's operation order
(coslam_amd/csrc/project_dev.h); get2DConvexHull / poly2Mask are LibVisualSLAM functions that are not in the reference tree: here the convex
hull (Andrew's monotone chain) and the CLOSED polygon test in EXACT arithmetic (fractions.Fraction over the f64 projections) -- the pixel
(x, y) is set when the integer point lies inside or on the hull polygon, and a hull with fewer than three vertices sets no pixel.

Inputs in this repository's terms (a scene dict): xy [nCams][N][2] (the undistorted pixel of a slot), state [nCams][N] (0 / 1: a feature of
the key frame), slot2map [nCams][N], mapPts [nMap][3], mapFlags [nMap] (CS_MAP_* bytes), mapCount, K / R [nCams][9], t [nCams][3], groups
(the key frame's record: lists of cameras in the order of discovery), frame.  Besides the answers every decision's MARGIN is returned.
Test infrastructure only."""
import math
from fractions import Fraction

import numpy as np

MAP_FALSE = 2   # CS_MAP_FALSE (include/coslam_hip.h)
DEFAULTS = (10, 0.5, 6.0)   # checkPossibleMergable(10, 0.5, Param::maxDistRatio), src/app/SL_CoSLAM.cpp:1380


def project(K, R, t, M):
    """project(K, R, t, M, m) in pu_project's operation order -> (m0, m1)"""
    K, R, t, M = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (K, R, t, M))
    X = ((R[0] * M[0] + R[1] * M[1]) + R[2] * M[2]) + t[0]
    Y = ((R[3] * M[0] + R[4] * M[1]) + R[5] * M[2]) + t[1]
    Z = ((R[6] * M[0] + R[7] * M[1]) + R[8] * M[2]) + t[2]
    u = (K[0] * X + K[1] * Y) + K[2] * Z
    v = (K[3] * X + K[4] * Y) + K[5] * Z
    w = (K[6] * X + K[7] * Y) + K[8] * Z
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(u / w), float(v / w)


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def exact_hull(pts):
    """the convex hull's vertices (counter-clockwise, Fractions) of pts (doubles), [] for fewer than three vertices"""
    P = sorted({(Fraction(float(x)), Fraction(float(y))) for x, y in pts})
    if len(P) < 3:
        return []
    lower, upper = [], []
    for p in P:
        while len(lower) >= 2 and _cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(P):
        while len(upper) >= 2 and _cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    Hh = lower[:-1] + upper[:-1]
    return Hh if len(Hh) >= 3 else []


def pixel_in_hull(hull, x, y):
    """poly2Mask's pixel (x, y): inside or ON the polygon -> (set, distance of the integer point to the nearest edge LINE)"""
    if not hull:
        return False, math.inf
    p = (Fraction(int(x)), Fraction(int(y)))
    inside, margin = True, math.inf
    for k in range(len(hull)):
        a, b = hull[k], hull[(k + 1) % len(hull)]
        c = _cross(a, b, p)
        if c < 0:
            inside = False
        margin = min(margin, abs(float(c)) / math.hypot(float(b[0] - a[0]), float(b[1] - a[1])))
    return inside, margin


def features(s, c):
    """the slots of camera c that are features of the key frame with a map point that is not false (:104-111, :150-155), in slot order"""
    out = []
    for k in range(s["N"]):
        if s["state"][c][k] not in (0, 1):
            continue
        m = int(s["slot2map"][c][k])
        if m < 0 or m >= s["mapCount"] or (s["mapFlags"][m] & MAP_FALSE):
            continue
        out.append((k, m))
    return out


def view_overlap_from_to(s, i, j, minInNum, minInAreaRatio):
    """checkViewOverlapFromTo (:98-171) -> dict(answer, nFeat (camera i's list), nInCam, inNum (-1: nInCam < minInNum), totalNum,
    image_margin, edge_margin, behind (in-image projections of points behind camera j), collinear)"""
    W, H = s["W"], s["H"]
    mapPts = features(s, i)                                           # :104-111
    ms, img_margin, behind = [], math.inf, 0
    Rj, tj = np.asarray(s["R"][j], dtype=np.float64).reshape(9), np.asarray(s["t"][j], dtype=np.float64).reshape(3)
    for _, m in mapPts:                                               # :120
        M = s["mapPts"][m]
        m0, m1 = project(s["K"][j], Rj, tj, M)                        # :124
        img_margin = min(img_margin, abs(m0), abs(m0 - W), abs(m1), abs(m1 - H))
        if m0 >= 0 and m0 < W and m1 >= 0 and m1 < H:                 # :125
            ms.append((m0, m1))                                       # :126-128
            behind += (Rj[6] * M[0] + Rj[7] * M[1]) + Rj[8] * M[2] + tj[2] < 0
    nInCam = len(ms)
    out = dict(answer=False, nFeat=len(mapPts), nInCam=nInCam, inNum=-1, totalNum=len(features(s, j)), image_margin=img_margin,
               edge_margin=math.inf, behind=behind, collinear=False)
    if nInCam >= minInNum:                                            # :136
        hull = exact_hull(ms)                                         # :139 get2DConvexHull, :143 poly2Mask
        out["collinear"] = not hull and nInCam >= 3
        inNum = totalNum = 0
        for k, _ in features(s, j):                                   # :150-155
            x, y = int(s["xy"][j][k][0]), int(s["xy"][j][k][1])       # :156-157 (toward zero, as C)
            inside, margin = pixel_in_hull(hull, x, y)
            out["edge_margin"] = min(out["edge_margin"], margin)
            inNum += inside                                           # :158-160
            totalNum += 1                                             # :161
        out["inNum"], out["totalNum"] = inNum, totalNum
        out["answer"] = bool(inNum > 50 or inNum >= minInAreaRatio * totalNum)   # :166
    return out


def cam_center(R, t):
    """getCamCenter: -R^T t"""
    R, t = np.asarray(R, dtype=np.float64).reshape(3, 3), np.asarray(t, dtype=np.float64).reshape(3)
    return np.array([-((R[0, k] * t[0] + R[1, k] * t[1]) + R[2, k] * t[2]) for k in range(3)])


def cam_dist(s, i, j):
    d = cam_center(s["R"][i], s["t"][i]) - cam_center(s["R"][j], s["t"][j])
    return float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))   # dist3 (:92)


def check_possible_mergable(s, minInNum=10, minInAreaRatio=0.5, maxCamDist=6.0, all_pairs=False):
    """checkPossibleMergable (:56-67) over s["groups"] -> dict(info [(f, i, g1, f, j, g2)], nFeat, nInCam, inNum, fromTo, camDist as
    cs_merge_candidates cut to the rig (-1 / 0 where a pair is not evaluated), detail {(i, j): view_overlap_from_to}, dist_margin)"""
    nC, groups = s["nCams"], s["groups"]
    gid = {c: g for g, cams in enumerate(groups) for c in cams}
    cache = s.setdefault("_from_to", {})   # (FromTo has no side effects: one evaluation of a pair serves every call with these thresholds)
    detail = {}
    for i in range(nC):
        for j in range(nC):
            if i != j and (all_pairs or (len(groups) > 1 and gid[i] != gid[j])):
                key = (i, j, minInNum, minInAreaRatio)
                if key not in cache:
                    cache[key] = view_overlap_from_to(s, i, j, minInNum, minInAreaRatio)
                detail[i, j] = cache[key]
    nFeat = [-1] * nC
    nInCam, inNum = np.full((nC, nC), -1, dtype=np.int64), np.full((nC, nC), -1, dtype=np.int64)
    fromTo = np.zeros((nC, nC), dtype=np.int64)
    for (i, j), d in detail.items():
        nFeat[i] = d["nFeat"]
        nInCam[i, j], inNum[i, j], fromTo[i, j] = d["nInCam"], d["inNum"], d["answer"]
    camDist = np.array([[cam_dist(s, i, j) if i != j else 0.0 for j in range(nC)] for i in range(nC)])
    info, dist_margin, beyond = [], math.inf, []
    for g1 in range(len(groups)):                                     # :59
        for g2 in range(g1 + 1, len(groups)):                         # :60
            for i in groups[g1]:                                      # :72-73
                for j in groups[g2]:                                  # :74-75
                    overlap = detail[i, j]["answer"] and detail[j, i]["answer"]   # :76, :173-177 (FromTo has no side effects)
                    near = not camDist[i, j] > maxCamDist             # :77, :93
                    dist_margin = min(dist_margin, abs(camDist[i, j] - maxCamDist))
                    if overlap and near:
                        info.append((s["frame"], i, g1, s["frame"], j, g2))   # :78-80
                    if overlap and not near:
                        beyond.append((i, j))
    return dict(info=info, nFeat=nFeat, nInCam=nInCam, inNum=inNum, fromTo=fromTo, camDist=camDist, detail=detail, dist_margin=dist_margin,
                beyond=beyond)


# ---- planted scenes (no rendering: the tables a key frame would leave) ---------------------------------------------------------------------
FOCAL = 500.0


def _pose(yaw, centre, rng, wobble):
    c, s_ = math.cos(yaw), math.sin(yaw)
    R = np.array([[c, 0.0, -s_], [0.0, 1.0, 0.0], [s_, 0.0, c]])     # the camera looks along (sin yaw, 0, cos yaw)
    if wobble:
        w = rng.uniform(-wobble, wobble, 3)
        a = np.linalg.norm(w)
        k = w / a
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R = (np.eye(3) + math.sin(a) * Kx + (1 - math.cos(a)) * Kx @ Kx) @ R
    centre = np.asarray(centre, dtype=np.float64)
    return R, (-(R @ centre) if centre.any() else np.zeros(3))


def planted_scene(seed, nCams, N, nMap, groups, yaws, plants, centres=None, far=(), exact=(), n_excluded=6, W=640, H=480, frame=7, Ks=None):
    """plants[c]: [(count, q, point_rect, pixel_rect, kind)] -- `count` features of camera c whose map points are the back-projections of
    uniform pixels of point_rect = (x0, y0, w, h) of camera q's image at depth 4..8 (kind "behind": at depth -8..-4, BEHIND camera q, the
    same pixel; kind "line": all on one exact image row of camera q, which must be an `exact` camera) and whose own pixels in camera c are
    uniform in pixel_rect (None: the whole image and 30 px around it).  Cameras on a unit circle looking outward along their yaw, a little
    wobbled; those in `exact` have R = I, t = 0 exactly (yaw 0); those in `far` stand 40 units above the others.  Sprinkled into EVERY camera, with map
    points that would project into its first plant's camera and pixels that would fall in its hull: n_excluded features each of a false
    point, a slot2map at / beyond the map count (below and beyond nMap), a state of -1 and of -2, and a slot without a map point."""
    rng = np.random.RandomState(seed)
    mapCount = nMap - nMap // 8
    K1 = np.array([FOCAL, 0, W / 2.0, 0, FOCAL, H / 2.0, 0, 0, 1.0])
    K = np.stack([K1] * nCams) if Ks is None else np.stack([np.asarray(k, dtype=np.float64).reshape(9) for k in Ks])
    Rs, ts = [], []
    for c in range(nCams):
        if c in exact:
            R, t = np.eye(3), np.zeros(3)
        else:
            # (far: 40 units to the side of every viewing direction -- no depth test, so a camera far out ALONG its axis would have the whole
            # rig in the cone behind it)
            cen = np.array([math.sin(yaws[c]), 40.0 if c in far else 0.0, math.cos(yaws[c])]) if centres is None else centres[c]
            R, t = _pose(yaws[c], cen + 0.05 * rng.randn(3), rng, 0.04)
        Rs.append(R), ts.append(t)
    mapPts = rng.uniform(-50, 50, (nMap, 3))           # (rows nobody names: anything)
    mapFlags = (rng.randint(0, 2, size=nMap) * rng.choice([0, 1, 4], size=nMap)).astype(np.uint8)   # dynamic / uncertain bits do not matter
    mapFlags &= np.uint8(0xFF ^ MAP_FALSE)
    xy = np.stack([np.stack([rng.uniform(-50, W + 50, N), rng.uniform(-50, H + 50, N)], axis=1) for _ in range(nCams)])
    state = np.full((nCams, N), -1, dtype=np.int32)
    state[rng.rand(nCams, N) < 0.3] = -2
    slot2map = np.full((nCams, N), -1, dtype=np.int32)
    rows_in, rows_out = list(rng.permutation(mapCount)), list(mapCount + rng.permutation(nMap - mapCount))
    free = [list(rng.permutation(N)) for _ in range(nCams)]

    def back(q, px, py, d):
        Kq = K[q]
        Xc = np.array([(px - Kq[2]) / Kq[0] * d, (py - Kq[5]) / Kq[4] * d, d])
        return Rs[q].T @ (Xc - ts[q])

    def put(c, q, prect, xrect, kind="ok", row=None, st=None, line=None):
        s = int(free[c].pop())
        r = int(rows_in.pop()) if row is None else row
        if kind == "line":                                   # exact camera: project() returns (K0 X / Z + K2, K4 Y / Z + K5) of M itself
            mapPts[r] = (rng.randint(-40, 40) / 16.0, line[0], line[1])
        else:
            d = rng.uniform(4, 8) * (-1 if kind == "behind" else 1)
            mapPts[r] = back(q, prect[0] + rng.uniform(0, prect[2]), prect[1] + rng.uniform(0, prect[3]), d)
        xy[c, s] = (rng.uniform(-30, W + 30), rng.uniform(-30, H + 30)) if xrect is None else \
            (xrect[0] + rng.uniform(0, xrect[2]), xrect[1] + rng.uniform(0, xrect[3]))
        state[c, s] = int(rng.randint(0, 2)) if st is None else st
        slot2map[c, s] = r
        return s, r

    for c in range(nCams):
        for count, q, prect, xrect, kind in plants[c]:
            line = (0.25, 4.0) if kind == "line" else None   # Y / Z exact in binary: one image row
            for _ in range(count):
                put(c, q, prect, xrect, kind, line=line)
        if not plants[c]:
            continue
        _, q, prect, xrect, _ = plants[c][0]
        prect = prect or (100, 100, 400, 300)
        mid = (W / 2 - 40, H / 2 - 40, 80, 80)
        for _ in range(n_excluded):
            _, r = put(c, q, prect, mid)                     # a false point
            mapFlags[r] |= MAP_FALSE
            put(c, q, prect, mid, row=int(rows_out.pop()))   # not a map point: at or beyond the map count
            s, _ = put(c, q, prect, mid)
            slot2map[c, s] = nMap + int(rng.randint(0, 50))  # ... and beyond the table
            put(c, q, prect, mid, st=-1)                     # not features of this frame
            put(c, q, prect, mid, st=-2)
            s, _ = put(c, q, prect, mid)
            slot2map[c, s] = -1                              # a feature without a map point
    return dict(nCams=nCams, N=N, nMap=nMap, W=W, H=H, mapCount=mapCount, mapPts=mapPts, mapFlags=mapFlags, xy=xy, state=state, slot2map=slot2map,
                K=K, R=np.stack([R.reshape(9) for R in Rs]), t=np.stack(ts), groups=[list(g) for g in groups], frame=frame)


SCENE_SEED = 20241017   # committed: the set below meets assert_scene_conditions with it (checked on the CPU by test_merge_cpu)
FULL = (20, 20, 600, 440)


def scene_set(seed=SCENE_SEED):
    """[(name, scene, (minInNum, minInAreaRatio, maxCamDist))]: 2, 3, 5, 8 and 16 cameras, 640 x 480, N 200-600, nMap 1000-2000"""
    sc = []
    tau = 2 * math.pi
    # two cameras back to back that hold each other's view: a candidate
    sc.append(("pair2", planted_scene(seed + 1, 2, 400, 1500, [[0], [1]], [0.0, math.pi],
                                      {0: [(150, 1, FULL, None, "ok")], 1: [(150, 0, FULL, None, "ok")]}), DEFAULTS))
    # three cameras: camera 0 exact (R = I, t = 0).  1 -> 0: a COLLINEAR set of 14 projections; 2 -> 0: a hull that holds exactly 20 of
    # camera 0's 40 features (inNum == ratio * totalNum, 20 <= 50); 0 -> 1 and 0 -> 2 from points BEHIND the target
    box, rest = (100.5, 100.5, 200, 200), (400, 50, 200, 380)
    sc.append(("three3", planted_scene(seed + 2, 3, 200, 1000, [[0], [1], [2]], [0.0, tau / 3, 2 * tau / 3],
                                       {0: [(20, 1, FULL, (110, 110, 180, 180), "behind"), (20, 2, FULL, rest, "behind")],
                                        1: [(14, 0, None, None, "line")],
                                        2: [(1, 0, (100.5, 100.5, 0, 0), None, "ok"), (1, 0, (300.5, 100.5, 0, 0), None, "ok"), (1, 0, (300.5, 300.5, 0, 0), None, "ok"),
                                            (1, 0, (100.5, 300.5, 0, 0), None, "ok"), (30, 0, box, None, "ok")]}, exact=(0,)), DEFAULTS))
    # five cameras 72 degrees apart, groups [0, 2, 1] (not ascending), [3], [4]; camera 4 far out.
    #   0 -> 3 holds, 3 -> 0 has nInCam = minInNum - 1 = 9: one way only.        2 -> 3: nInCam = minInNum = 10 exactly.
    #   0 -> 4: a hull that holds exactly 50 of camera 4's 160 features (ratio unmet).   1 -> 4: one that holds 51; 4 -> 1 holds: an overlap
    #   both ways, beyond maxCamDist
    sq = [(100.5, 100.5), (300.5, 100.5), (300.5, 300.5), (100.5, 300.5)]   # (no edge line through integer points)
    corners = lambda q, pts: [(1, q, (x, y, 0, 0), None, "ok") for x, y in pts]   # noqa: E731
    sc.append(("edge5", planted_scene(seed + 3, 5, 600, 2000, [[0, 2, 1], [3], [4]], [k * tau / 5 for k in range(5)],
                                      {0: [(200, 3, FULL, None, "ok")] + corners(4, sq) + [(20, 4, (120, 120, 160, 160), None, "ok")],
                                       1: corners(4, sq + [(400.5, 200.25)]) + [(20, 4, (120, 120, 160, 160), None, "ok")],
                                       2: [(10, 3, (200, 150, 200, 150), None, "ok")],
                                       3: [(9, 0, FULL, None, "ok"), (150, 4, FULL, None, "ok")],
                                       4: [(50, 1, FULL, (120, 120, 160, 160), "ok"), (1, 1, FULL, (340, 190, 20, 20), "ok"),
                                           (109, 1, FULL, (450, 20, 170, 440), "ok")]}, far=(4,), n_excluded=4), DEFAULTS))
    # eight cameras, ONE group: two clusters of four that look the same way
    y8 = [0.0] * 4 + [math.pi] * 4
    p8 = {c: [(60, (c + 1) % 4 + 4 * (c // 4), (120, 90, 400, 300), None, "ok"), (15, (c + 4) % 8, FULL, None, "ok")] for c in range(8)}
    sc.append(("onegroup8", planted_scene(seed + 4, 8, 300, 1500, [list(range(8))], y8, p8, n_excluded=3), DEFAULTS))
    # sixteen singleton groups that all look the same way from one place: 120 group pairs; camera 5 far out
    cen16 = [np.array([0.1 * (c % 4), 0.1 * (c // 4), -40.0 if c == 5 else 0.0]) for c in range(16)]
    p16 = {c: [(70, (c + 3) % 16, (170, 130, 300, 220), (240, 190, 160, 100), "ok")] for c in range(16)}
    sc.append(("singletons16", planted_scene(seed + 5, 16, 200, 2000, [[c] for c in range(16)], [0.0] * 16, p16, centres=cen16, n_excluded=2),
               DEFAULTS))
    return sc


def scene_results(scenes):
    """{(name, all_pairs): check_possible_mergable(...)}"""
    return {(name, ap): check_possible_mergable(s, *par, all_pairs=ap) for name, s, par in scenes for ap in (False, True)}


def assert_scene_conditions(scenes, results):
    """what the scene set must exercise, asserted on the RESTATEMENT's output, and the margins that make the decisions safe in f64"""
    seen = dict(candidate=0, one_way=0, beyond=0, at_min_minus_1=0, at_min=0, in50=0, in51=0, ratio_exact=0, collinear=0, behind=0,
                not_ascending=0, one_group=0, many_infos=0, excluded=0)
    for name, s, par in scenes:
        r, ra = results[name, False], results[name, True]
        seen["candidate"] += len(r["info"]) > 0
        seen["beyond"] += len(r["beyond"]) > 0
        seen["not_ascending"] += any(g != sorted(g) for g in s["groups"])
        seen["one_group"] += len(s["groups"]) == 1 and not r["info"] and not r["detail"] and len(ra["detail"]) == s["nCams"] * (s["nCams"] - 1)
        seen["many_infos"] += len(s["groups"]) == 16 and len(r["info"]) > 16
        assert r["dist_margin"] >= 1e-6 and ra["dist_margin"] >= 1e-6, (name, r["dist_margin"])
        for (i, j), d in ra["detail"].items():
            assert d["image_margin"] >= 1e-6, (name, i, j, d["image_margin"])
            assert d["edge_margin"] >= 1e-6, (name, i, j, d["edge_margin"])
            back = ra["detail"][j, i]
            seen["one_way"] += d["answer"] and not back["answer"]
            seen["at_min_minus_1"] += d["nInCam"] == par[0] - 1
            seen["at_min"] += d["nInCam"] == par[0]
            unmet = d["inNum"] < par[1] * d["totalNum"]
            seen["in50"] += d["inNum"] == 50 and unmet and not d["answer"]
            seen["in51"] += d["inNum"] == 51 and unmet and d["answer"]
            seen["ratio_exact"] += 0 < d["inNum"] <= 50 and d["inNum"] == par[1] * d["totalNum"] and d["answer"]
            seen["collinear"] += d["collinear"] and d["nInCam"] >= par[0] and d["inNum"] == 0
            seen["behind"] += d["behind"] > 0
        # the excluded kinds are among the slots of every camera that has a plant
        for c in range(s["nCams"]):
            st, m = s["state"][c], s["slot2map"][c]
            live = (st == 0) | (st == 1)
            ok = (m >= 0) & (m < s["mapCount"])
            false_ = live & ok & ((s["mapFlags"][np.clip(m, 0, s["nMap"] - 1)] & MAP_FALSE) != 0)
            seen["excluded"] += bool(false_.any() and (live & (m >= s["mapCount"]) & (m < s["nMap"])).any() and (live & (m >= s["nMap"])).any()
                                     and ((st == -1) & ok).any() and ((st == -2) & ok).any())
    assert all(v >= 1 for v in seen.values()), seen
    return seen


# ---- the lattice scene: the closed-polygon rule with nothing rounded ---------------------------------------------------------------------
LATTICE_HULL = [(10, 10), (50, 10), (70, 40), (50, 70), (10, 70), (0, 40)]       # camera 0's points M = (u, v, 1) project to (u, v) in camera 1
LATTICE_INNER = [(20, 20), (30, 40), (50, 40), (30, 10), (60, 25), (5, 25), (40, 70)]   # inside or on an edge: no vertices
# camera 1's feature pixels (as stored: (int) truncates toward zero) and whether the pixel is set -- counted by hand:
#   the six vertices: set.  (30, 10) bottom edge, (60, 25) on (50, 10)-(70, 40), (5, 25) on (0, 40)-(10, 10), (60, 55) on (70, 40)-(50, 70): set.
#   (30, 11), (59, 25), (6, 25), (35, 40) inside: set.  (30, 9), (61, 25), (4, 25), (60, 56), (71, 40), (-0.5 -> 0, 39) [(0, 39): left of
#   (0, 40)-(10, 10)], (200, 200): not set.  (0.9 -> 0, 40.9 -> 40) is the vertex (0, 40): set.
LATTICE_PIXELS = [((10.0, 10.0), 1), ((50.5, 10.9), 1), ((70.0, 40.0), 1), ((50.0, 70.2), 1), ((10.9, 70.9), 1), ((0.9, 40.9), 1),
                  ((30.7, 10.2), 1), ((60.0, 25.0), 1), ((5.5, 25.5), 1), ((60.1, 55.9), 1),
                  ((30.0, 11.0), 1), ((59.9, 25.0), 1), ((6.0, 25.0), 1), ((35.0, 40.0), 1),
                  ((30.0, 9.9), 0), ((61.0, 25.0), 0), ((4.9, 25.0), 0), ((60.0, 56.0), 0), ((71.0, 40.0), 0), ((-0.5, 39.0), 0), ((200.0, 200.0), 0)]
LATTICE_IN_NUM = 14   # by hand: 6 vertices + 4 on edges + 4 inside
LATTICE_PARAMS = (5, 0.5, 6.0)


def lattice_scene():
    """two cameras, two groups; camera 1 has K = I, R = I, t = 0: every projection and every cross product is an exact integer"""
    N, nMap, W, H = 64, 100, 640, 480
    pts = LATTICE_HULL + LATTICE_INNER
    mapPts = np.zeros((nMap, 3))
    state, slot2map = np.full((2, N), -1, dtype=np.int32), np.full((2, N), -1, dtype=np.int32)
    xy = np.zeros((2, N, 2))
    for k, (u, v) in enumerate(pts):                       # camera 0: slots 3, 5, 7, ... -> map rows 2 k
        mapPts[2 * k] = (u, v, 1.0)
        state[0, 3 + 2 * k], slot2map[0, 3 + 2 * k], xy[0, 3 + 2 * k] = k % 2, 2 * k, (100.0 + k, 50.0)
    for k, ((x, y), _) in enumerate(LATTICE_PIXELS):       # camera 1: slots 1, 3, 5, ... -> map rows 41 + k (points far off camera 0's image)
        mapPts[41 + k] = (1e4 + k, 1e4, 1.0)
        state[1, 1 + 2 * k], slot2map[1, 1 + 2 * k], xy[1, 1 + 2 * k] = k % 2, 41 + k, (x, y)
    K = np.stack([np.array([FOCAL, 0, 320.0, 0, FOCAL, 240.0, 0, 0, 1.0]), np.eye(3).reshape(9)])
    R = np.stack([np.eye(3).reshape(9)] * 2)
    t = np.array([[0.5, 0.0, 0.0], [0.0, 0.0, 0.0]])
    return dict(nCams=2, N=N, nMap=nMap, W=W, H=H, mapCount=90, mapPts=mapPts, mapFlags=np.zeros(nMap, dtype=np.uint8), xy=xy, state=state,
                slot2map=slot2map, K=K, R=R, t=t, groups=[[0], [1]], frame=3)
