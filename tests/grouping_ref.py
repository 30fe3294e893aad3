"""Restatement of CoSLAM::getViewOverlapCosts and CoSLAM::cameraGrouping (reference src/app/SL_CoSLAM.cpp:1543-1697) in numpy / pure
Python, branch by branch with the reference's line numbers, written from the reference's text.  get2DConvexHull / getPolyArea are
LibVisualSLAM functions that are not in the reference tree: here the convex hull (Andrew's monotone chain) and its shoelace area in EXACT
arithmetic (fractions.Fraction over the doubles), zero for fewer than three points or a collinear set.

Inputs in this repository's terms: pointFeat [nMap][nCams] (slot of the feature of THIS frame or < 0), mapFlags [nMap] (CS_MAP_* bytes),
xy[c] [N][2] (the undistorted pixel of camera c's slot), mapCount (rows below it are map points), rows (an optional list of map indices:
the frame's current points).  Test infrastructure only."""
from fractions import Fraction

import numpy as np

MAP_FALSE = 2   # CS_MAP_FALSE (include/coslam_hip.h)


def exact_hull_area(pts):
    """area of the convex hull of pts (k x 2 doubles), exact until the final conversion to float"""
    P = sorted({(Fraction(float(x)), Fraction(float(y))) for x, y in pts})
    if len(P) < 3:
        return 0.0

    def cross(o, a, b):
        return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])

    lower, upper = [], []
    for p in P:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(P):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    H = lower[:-1] + upper[:-1]
    if len(H) < 3:
        return 0.0
    s = Fraction(0)
    for k in range(len(H)):
        a, b = H[k], H[(k + 1) % len(H)]
        s += a[0] * b[1] - b[0] * a[1]
    return float(abs(s) / 2)


def shared_points(pointFeat, mapFlags, xy, mapCount=None, rows=None):
    """:1551-1595 -> nShare [nCams][nCams] ints and sharedPoints[i][j] (lists of pixels of camera i)"""
    pointFeat = np.asarray(pointFeat)
    nMap, nC = pointFeat.shape
    mapCount = nMap if mapCount is None else min(int(mapCount), nMap)
    nShare = np.zeros((nC, nC), dtype=np.int32)                       # :1545-1546
    shared = [[[] for _ in range(nC)] for _ in range(nC)]             # :1549-1558
    walk = range(mapCount) if rows is None else [int(r) for r in rows if 0 <= int(r) < mapCount]
    held = pointFeat >= 0
    nVis = held.sum(axis=1)
    for p in walk:                                                    # :1561 (curMapPts in map order)
        if nVis[p] == 1 or (mapFlags is not None and mapFlags[p] & MAP_FALSE):   # :1563 (numVisCam == 1 || isFalse())
            continue
        viewIds = [c for c in range(nC) if held[p, c]]                # :1568-1575 (fp && fp->f == curFrame)
        for a in range(len(viewIds)):                                 # :1577
            iCam = viewIds[a]
            for b in range(a + 1, len(viewIds)):                      # :1579
                jCam = viewIds[b]
                nShare[iCam, jCam] += 1                               # :1581
                nShare[jCam, iCam] += 1                               # :1582
                shared[iCam][jCam].append(tuple(xy[iCam][pointFeat[p, iCam]]))   # :1590-1591
                shared[jCam][iCam].append(tuple(xy[jCam][pointFeat[p, jCam]]))   # :1592-1593
    return nShare, shared


def view_overlap_costs(pointFeat, mapFlags, xy, W, H, minOverlapNum, minOverlapAreaRatio, mapCount=None, rows=None, with_area=True):
    """getViewOverlapCosts (:1543-1630) -> vcosts [nC][nC] doubles, nShare, area [nC][nC] (the exact hull areas, :1597-1603).
    with_area=False: the areas are not computed -- allowed only where they cannot matter (minOverlapAreaRatio <= 0: no area is < 0)."""
    nShare, shared = shared_points(pointFeat, mapFlags, xy, mapCount, rows)
    nC = nShare.shape[0]
    assert with_area or minOverlapAreaRatio <= 0
    area = np.zeros((nC, nC))
    if with_area:
        for i in range(nC):                                           # :1597-1603
            for j in range(nC):
                if i != j:
                    area[i, j] = exact_hull_area(shared[i][j])
    vcosts = np.zeros((nC, nC))
    for i in range(nC):                                               # :1605
        vcosts[i, i] = -1                                             # :1606
        for j in range(i + 1, nC):                                    # :1607
            if nShare[i, j] < minOverlapNum:                          # :1608
                vcosts[i, j] = vcosts[j, i] = -1                      # :1609-1610
            else:
                area1, area2 = area[i, j], area[j, i]                 # :1613-1614
                iArea = float(W) * float(H)                           # :1616-1617 (one image size for the rig)
                jArea = float(W) * float(H)
                if area1 < minOverlapAreaRatio * iArea or area2 < minOverlapAreaRatio * jArea:   # :1619-1620
                    vcosts[i, j] = vcosts[j, i] = -1                  # :1621-1622
                else:
                    vcosts[i, j] = nShare[i, j]                       # :1624
                    vcosts[j, i] = vcosts[i, j]                       # :1625
    return vcosts, nShare, area


def cam_center(R, t):
    """getCamCenter (src/slam/SL_SLAMHelper.cpp:197-199): -R^T t"""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    return np.array([-((R[0, k] * t[0] + R[1, k] * t[1]) + R[2, k] * t[2]) for k in range(3)])


def cam_dist(R1, t1, R2, t2):
    d = cam_center(R1, t1) - cam_center(R2, t2)
    return float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))


def init_cam_translation(Rs, ts):
    """m_initCamTranslation (:280-290): the mean pairwise distance of the camera centres"""
    s, n = 0.0, 0
    for i in range(len(Rs)):
        for j in range(i + 1, len(Rs)):
            s += cam_dist(Rs[i], ts[i], Rs[j], ts[j])
            n += 1
    return s / n if n else 0.0


def components(vcosts):
    """:1659-1695: connected components over cost > 0 with the explicit stack -> groups (lists in the order of discovery), groupId"""
    vcosts = np.asarray(vcosts)
    nC = vcosts.shape[0]
    flag = [0] * nC                                                   # :1662
    groups, groupId = [], [-1] * nC
    for i in range(nC):                                               # :1664
        if flag[i] == 0:                                              # :1665
            CON, VQ = [i], [i]                                        # :1667-1669
            flag[i] = 1                                               # :1670
            while VQ:                                                 # :1672
                iCam = VQ.pop()                                       # :1674-1675 (the LAST pushed)
                for j in range(nC):                                   # :1678
                    if j != iCam and flag[j] == 0 and vcosts[iCam, j] > 0:   # :1679-1680
                        CON.append(j)                                 # :1681
                        VQ.append(j)                                  # :1682
                        flag[j] = 1                                   # :1683
            for k in CON:                                             # :1688-1691
                groupId[k] = len(groups)
            groups.append(CON)                                        # :1692
    return groups, groupId


def camera_grouping(pointFeat, mapFlags, xy, W, H, Rs, ts, initCamTranslation, maxDistRatio=6.0, minOverlapNum=0, minOverlapAreaRatio=0.0,
                    mapCount=None, rows=None, with_area=True):
    """cameraGrouping (:1632-1697; the reference's own call has minOverlapNum = 0, minOverlapAreaRatio = 0.0)
    -> dict(groups, groupId, vcosts (after the distance cut), nShare, area, cut (the pairs the distance removed))"""
    nC = np.asarray(pointFeat).shape[1]
    if nC == 1:                                                       # :1633-1634
        return dict(groups=[[0]], groupId=[0], vcosts=np.full((1, 1), -1.0), nShare=np.zeros((1, 1), dtype=np.int32), area=np.zeros((1, 1)),
                    cut=[])
    vcosts, nShare, area = view_overlap_costs(pointFeat, mapFlags, xy, W, H, minOverlapNum, minOverlapAreaRatio, mapCount, rows, with_area)   # :1635
    cut = []
    for i in range(nC):                                               # :1638
        for j in range(i + 1, nC):                                    # :1640
            if vcosts[i, j] > 0 and cam_dist(Rs[i], ts[i], Rs[j], ts[j]) > initCamTranslation * maxDistRatio:   # :1645-1647
                vcosts[i, j] = vcosts[j, i] = -1                      # :1649-1650
                cut.append((i, j))
    groups, groupId = components(vcosts)
    return dict(groups=groups, groupId=groupId, vcosts=vcosts, nShare=nShare, area=area, cut=cut)


# ---- planted scenes for the tests (no rendering: the tables a frame would leave, built from a camera graph) --------------------------------
def planted_scene(seed, nCams, N, nMap, W, H, plants, far=(), far_factor=40.0, n_false=40, n_single=60, n_beyond=25):
    """plants: [(cameras, count, rect or None)] -- `count` map points held by every camera of `cameras` in this frame, their pixels uniform
    in the image or in rect = (x0, y0, w, h).  Sprinkled in: n_false points that two cameras hold but that are CS_MAP_FALSE, n_single points
    that one camera holds, n_beyond shared points in rows at or beyond the map count (not map points: to be ignored).  Cameras on a circle
    looking at random; those in `far` moved far_factor radii out AFTER m_initCamTranslation was taken.
    -> dict(pointFeat, mapFlags, xy [nCams][N][2], mapCount, R [nCams][9], t [nCams][3], initCamTranslation, rows (the current-points list))"""
    rng = np.random.RandomState(seed)
    mapCount = nMap - nMap // 10
    pointFeat = np.full((nMap, nCams), -1, dtype=np.int32)
    mapFlags = (rng.randint(0, 2, size=nMap) * rng.choice([0, 1, 4], size=nMap)).astype(np.uint8)   # dynamic / uncertain bits do not matter
    mapFlags &= np.uint8(0xFF ^ MAP_FALSE)
    xy = np.stack([np.stack([rng.uniform(-50, W + 50, N), rng.uniform(-50, H + 50, N)], axis=1) for _ in range(nCams)])   # (unused slots: anything)
    free = [list(rng.permutation(N)) for _ in range(nCams)]
    rows_in = list(rng.permutation(mapCount))
    rows_out = list(mapCount + rng.permutation(nMap - mapCount))

    def put(row, cams, rect):
        for c in cams:
            s = int(free[c].pop())
            pointFeat[row, c] = s
            if rect is None:
                xy[c, s] = rng.uniform(0, W), rng.uniform(0, H)
            else:
                xy[c, s] = rect[0] + rng.uniform(0, rect[2]), rect[1] + rng.uniform(0, rect[3])

    for cams, count, rect in plants:
        for _ in range(count):
            put(int(rows_in.pop()), cams, rect)
    for _ in range(n_false if nCams > 1 else 0):
        r = int(rows_in.pop())
        put(r, tuple(rng.choice(nCams, 2, replace=False)), None)
        mapFlags[r] |= MAP_FALSE
    for _ in range(n_single):
        put(int(rows_in.pop()), (int(rng.randint(nCams)),), None)
    for _ in range(n_beyond if nCams > 1 else 0):
        put(int(rows_out.pop()), tuple(rng.choice(nCams, 2, replace=False)), None)
    Rs, ts, Cs = [], [], []
    for c in range(nCams):
        Q, _ = np.linalg.qr(rng.randn(3, 3))
        if np.linalg.det(Q) < 0:
            Q[:, 0] = -Q[:, 0]
        a = 2 * np.pi * c / nCams
        Cs.append(np.array([3.0 * np.cos(a), 0.2 * rng.randn(), 3.0 * np.sin(a)]))
        Rs.append(Q)
    ts = [-(R @ C) for R, C in zip(Rs, Cs)]
    init = init_cam_translation(Rs, ts)
    for c in far:
        Cs[c] = Cs[c] * far_factor
        ts[c] = -(Rs[c] @ Cs[c])
    held = (pointFeat >= 0).any(axis=1)
    rows = np.array([r for r in range(mapCount) if held[r] and not (mapFlags[r] & MAP_FALSE)], dtype=np.int32)   # cs_register_list_current_dev's list
    return dict(pointFeat=pointFeat, mapFlags=mapFlags, xy=xy, mapCount=mapCount, R=np.stack([R.reshape(9) for R in Rs]), t=np.stack(ts),
                initCamTranslation=init, rows=rows, W=W, H=H, N=N, nMap=nMap, nCams=nCams)


SCENE_SEED = 20240817   # committed: the set below meets test_grouping_gpu's conditions with it (checked on the CPU by test_grouping_cpu)
THRESHOLDS = (10, 0.2)  # the positive thresholds every scene is also run with


def scene_set(seed=SCENE_SEED):
    """the GPU tests' scenes: chains, a star, the issue's 8-camera plant, two cliques joined by one bridge pair and an isolated camera"""
    W, H, N = 640, 480, 2000
    small = (300.0, 200.0, 40.0, 40.0)
    sc = []
    sc.append(("pair", planted_scene(seed + 1, 2, N, 6000, W, H, [((0, 1), 1500, None)])))
    sc.append(("chain3", planted_scene(seed + 2, 3, N, 7000, W, H, [((0, 2), 300, None), ((2, 1), 300, None)])))
    sc.append(("star5", planted_scene(seed + 3, 5, N, 9000, W, H, [((2, 0), 250, None), ((2, 1), 200, None), ((2, 3), 350, None), ((2, 4), 150, None),
                                                                   ((0, 2, 4), 100, None)])))
    sc.append(("plant8", planted_scene(seed + 4, 8, N, 12000, W, H, [((0, 2), 300, None), ((2, 1), 300, None), ((3, 4), 10, None), ((4, 5), 200, small),
                                                                     ((5, 6), 9, None), ((6, 7), 250, None)], far=(7,), n_false=0)))
    sc.append(("cliques13", planted_scene(seed + 5, 13, N, 16000, W, H, [(tuple(range(0, 6)), 400, None), (tuple(range(6, 12)), 500, None),
                                                                         ((5, 6), 60, small), ((0, 3), 200, None), ((7, 9, 11), 150, None)])))
    chain = [((c, c + 1), [400, 10, 350, 9, 500, 300, 250, 10, 450, 8, 320, 280, 1200, 260, 240][c], small if c in (5, 11) else None)
             for c in range(15)]
    sc.append(("chain16", planted_scene(seed + 6, 16, N, 20000, W, H, chain + [((0, 15), 3, None), ((2, 9), 5, None)], far=(13, 14), n_false=0)))
    return sc


def scene_results(scenes):
    """the restatement over the set: {(name, thresholds): camera_grouping(...)} for (0, 0.0) and THRESHOLDS"""
    out = {}
    for name, s in scenes:
        for th in ((0, 0.0), THRESHOLDS):
            out[name, th] = camera_grouping(s["pointFeat"], s["mapFlags"], s["xy"], s["W"], s["H"], s["R"], s["t"], s["initCamTranslation"], 6.0,
                                            th[0], th[1], s["mapCount"])
    return out


def assert_scene_conditions(scenes, results):
    """what the scene set must exercise, asserted on the RESTATEMENT's output (a set that exercises nothing cannot pass)"""
    sizes = set()
    not_ascending = cut_count = cut_area = cut_dist = at_exactly = 0
    for name, s in scenes:
        WH = float(s["W"]) * s["H"]
        for th in ((0, 0.0), THRESHOLDS):
            r = results[name, th]
            sizes.add(len(r["groups"]))
            not_ascending += sum(1 for g in r["groups"] if g != sorted(g))
            nC = s["nCams"]
            for i in range(nC):
                for j in range(i + 1, nC):
                    n = int(r["nShare"][i, j])
                    if th[1] > 0:
                        if 0 < n < th[0]:
                            cut_count += 1
                        if n == th[0]:
                            at_exactly += 1
                        if n >= th[0] and (r["area"][i, j] < th[1] * WH or r["area"][j, i] < th[1] * WH):
                            cut_area += 1
                        if n >= th[0]:   # no area near its threshold: the equality of vcosts does not hang on the area's tolerance
                            assert abs(r["area"][i, j] - th[1] * WH) > 1e-6 * WH and abs(r["area"][j, i] - th[1] * WH) > 1e-6 * WH, (name, i, j)
            cut_dist += sum(1 for (i, j) in r["cut"] if r["nShare"][i, j] > 0)
    assert not_ascending >= 1 and 1 in sizes and 2 in sizes and max(sizes) >= 4, (not_ascending, sizes)
    assert cut_count >= 1 and cut_area >= 1 and cut_dist >= 1 and at_exactly >= 1, (cut_count, cut_area, cut_dist, at_exactly)
