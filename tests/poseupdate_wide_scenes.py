"""Map-point scenes at ANY camera count in the array layout of tests/golden/update_points_golden.npz and classify_golden.npz (plain
numpy; tests/cxx/ref_update_points_test.cpp and ref_classify_test.cpp are the recipes' models).  The reference stops at 13 cameras
(SLAM_MAX_NUM); 14 and 16 cameras -- 16 is the only count at which two lanes per (camera, point) pair and four lanes per camera fill the
wave, and checkUnify's flat rotation array holds its 64th view -- take the C oracle as the expectation, which the wide fixtures hold to
the reference at 7..13 cameras.

A scene: the rig of the wide golden modes (per-camera offset and yaw scaled by 4 / (nCams - 1)), every odd camera standing still for
the older half of the history with bit-identical poses; nP points, every fourth with a feature in every camera, half seen by most, the
rest by two cameras or fewer; chains of 1 .. H + 8 nodes, so some are older than the ring and the walk bound cuts them; pairs for
checkUnify: the halves of one point, neighbours, and two different fully seen points (4 * nCams candidate views).  `update_scenes` /
`classify_scenes` return {"n_scenes", "s<i>_<array>"} like the loaded fixtures, the *_ref arrays filled by the oracle."""
import numpy as np

CAMERA_COUNTS = (14, 16)
SIGMA = 10.0      # Const::PIXEL_ERR_VAR
PIXEL_VAR = 12.0  # CoSLAM::poseUpdate: mapPointsClassify(12.0)


def _rodrigues(w):
    th = np.linalg.norm(w)
    k = w / th if th > 0 else np.zeros(3)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def make_scene(nC, seed, nP=32, H=32):
    """one scene: the arrays both layouts share, plus the classification's per-point state"""
    rng = np.random.default_rng(seed)
    cur, N = 500 + nC, nP
    rig = 4.0 / (nC - 1)
    K, iK = np.zeros((nC, 9)), np.zeros((nC, 9))
    for c in range(nC):
        Kc = np.array([[515 + 15 * rng.random(), 0.3 * (c % 2), 320 + 4 * rng.normal()], [0, 512 + 15 * rng.random(), 240 + 4 * rng.normal()], [0, 0, 1]])
        K[c], iK[c] = Kc.reshape(9), np.linalg.inv(Kc).reshape(9)
    hR, hT = np.zeros((nC, H, 9)), np.zeros((nC, H, 3))
    for c in range(nC):
        cs = c * rig
        for j in range(H):
            if c % 2 == 1 and j > H // 2:   # stood still: bit-identical poses, equal angles -- the first node of the walk wins
                hR[c, j], hT[c, j] = hR[c, H // 2], hT[c, H // 2]
                continue
            jj = min(j, H // 2) if c % 2 == 1 else j
            R = _rodrigues(np.array([0.01 * cs + 0.002 * rng.normal(), 0.12 * cs - 0.006 * jj, 0.002 * jj + 0.002 * rng.normal()]))
            pos = np.array([1.5 * cs - 0.09 * jj, 0.05 * cs + 0.01 * jj, -0.03 * jj]) + 0.004 * rng.normal(size=3)
            hR[c, j], hT[c, j] = R.reshape(9), -R @ pos
    hXY = np.zeros((nC, H, 2 * N))
    span = np.full((nC, 2 * N), -1, np.int32)
    fstat = np.ones((nC, N), np.uint8)
    pf = np.full((nP, nC), -1, np.int32)
    M0, cov0 = np.zeros((nP, 3)), np.zeros((nP, 9))
    flags, lastF, isCur = np.zeros(nP, np.uint8), np.zeros(nP, np.int32), np.zeros(nP, np.uint8)
    newPt, sfn, firstF = np.zeros(nP, np.uint8), np.zeros(nP, np.int32), np.zeros(nP, np.int32)
    firstKey = cur - 12
    for p in range(nP):
        X = np.array([-2 + 7 * rng.random(), -1.5 + 3 * rng.random(), 7 + 6 * rng.random()])
        moving, garbage = p % 8 == 5, p % 16 == 7
        vel = np.array([0.05 * (1 if rng.random() < 0.5 else -1), 0.02 * rng.normal(), 0.02 * rng.normal()]) if moving else np.zeros(3)
        M0[p] = X + np.array([0.05, 0.05, 0.1]) * rng.normal(size=3)
        A = 0.05 * rng.normal(size=(3, 3))
        cov0[p] = (A @ A.T + 1e-6 * np.eye(3)).reshape(9)
        u = rng.random()
        flags[p] = (1 if (moving or u < 0.15) else (2 if u < 0.2 else 0)) | (4 if rng.random() < 0.4 else 0)
        lastF[p] = firstKey - int(3 * rng.random()) if rng.random() < 0.12 else cur - int(4 * rng.random())
        isCur[p] = rng.random() < 0.75
        newPt[p] = rng.random() < 0.5
        firstF[p] = cur - 12 if rng.random() < 0.3 else cur - 45
        sfn[p] = 50 if rng.random() < 0.3 else int(40 * rng.random())
        if p % 4 == 0:
            sees = np.ones(nC, bool)
        elif p % 4 == 3:
            sees = np.zeros(nC, bool)
            sees[rng.permutation(nC)[:p % 3]] = True   # none, one or two cameras
        else:
            sees = rng.random(nC) < 0.7
        for c in np.nonzero(sees)[0]:
            L = 1 + int(rng.random() * (H + 8))   # (longer than the ring: the older nodes are not in the history)
            if p % 4 == 0 and L < 2:
                L = 2
            pf[p, c] = p
            span[c, p], span[c, N + p] = cur - L + 1, cur
            fstat[c, p] = rng.random() >= 0.35
            for j in range(min(L, H)):
                R, t, Kc = hR[c, j].reshape(3, 3), hT[c, j], K[c].reshape(3, 3)
                Xc = R @ (X - vel * j) + t
                assert Xc[2] > 0
                m = (Kc @ Xc)[:2] / Xc[2] + 0.6 * rng.normal(size=2) + (60 * rng.normal(size=2) if garbage else 0)
                hXY[c, j, p], hXY[c, j, N + p] = m
    seen = (pf >= 0).sum(axis=1)
    pairs = []
    for p in range(nP - 1):
        if seen[p] >= 2:   # the halves of one point's cameras, dealt out alternately
            cams = np.nonzero(pf[p] >= 0)[0]
            h1, h2 = np.zeros(nC, np.uint8), np.zeros(nC, np.uint8)
            h1[cams[0::2]], h2[cams[1::2]] = 1, 1
            pairs.append((p, p, h1, h2, M0[p], M0[p] + np.array([0.02, -0.015, 0.03])))
        q = p + 1
        if seen[p] >= 1 and seen[q] >= 1:
            pairs.append((p, q, (pf[p] >= 0).astype(np.uint8), (pf[q] >= 0).astype(np.uint8), M0[p], M0[q]))
        q = p + 4
        if q < nP and seen[p] == nC and seen[q] == nC:   # two different points every camera sees
            pairs.append((p, q, np.ones(nC, np.uint8), np.ones(nC, np.uint8), M0[p], M0[q]))
    return dict(K=K, iK=iK, histR=hR, histT=hT, histXY=hXY, trackSpan=span, featStatic=fstat, pointFeat=pf, M0=M0, cov0=cov0, flags=flags,
                lastFrame=lastF, isCurrent=isCur, firstKey=np.int32(firstKey), curFrame=np.int32(cur), sigma=np.float64(SIGMA),
                refine_select=(seen >= 2).astype(np.uint8),
                unify_pts=np.array([(a, b) for a, b, *_ in pairs], np.int32), unify_has1=np.stack([x[2] for x in pairs]),
                unify_has2=np.stack([x[3] for x in pairs]), unify_M1=np.stack([x[4] for x in pairs]), unify_M2=np.stack([x[5] for x in pairs]),
                newPt=newPt, staticFrameNum=sfn, firstFrame=firstF, pixelVar=np.float64(PIXEL_VAR),
                featFrame=np.where(pf >= 0, cur, -1).astype(np.int32), featFirst=np.where(pf >= 0, span[:, :N].T, -1).astype(np.int32))


def feature_refs(S):
    """the scene's features as references {slot, frame, first, seg} with no segment linked behind, and an empty pool: what the
    `_ref` entry points read instead of pointFeat + trackSpan"""
    pf, cur = S["pointFeat"], int(S["curFrame"])
    nP, nC = pf.shape
    ref = np.full((nP, nC, 4), -1, np.int32)
    ref[:, :, 1] = np.where(pf >= 0, cur, -1)
    ref[:, :, 0], ref[:, :, 2] = pf, S["featFirst"]
    return ref, np.full((nC, 2 * nP, 4), -1, np.int32)


def _update_expectations(S):
    import oracle

    out = dict(S)
    M, cov = S["M0"].copy(), S["cov0"].copy()
    oracle.update_new_poses_points(S["K"], S["iK"], S["histR"], S["histT"], S["histXY"], S["trackSpan"], S["featStatic"], S["pointFeat"], M, cov,
                                   S["flags"], float(S["sigma"]), lastFrame=S["lastFrame"], isCurrent=S["isCurrent"], firstKeyFrame=int(S["firstKey"]))
    out["M_ref"], out["cov_ref"] = M, cov
    M, cov = S["M0"].copy(), S["cov0"].copy()
    oracle.refine_map_points(S["K"], S["iK"], S["histR"], S["histT"], S["histXY"], S["trackSpan"], S["pointFeat"], M, cov, float(S["sigma"]),
                             select=S["refine_select"])
    out["M_refine"], out["cov_refine"] = M, cov
    nU, pf = len(S["unify_pts"]), S["pointFeat"]
    ok, uM, ucov = np.zeros(nU, np.uint8), np.zeros((nU, 3)), np.zeros((nU, 9))
    for q in range(nU):
        p1, p2 = S["unify_pts"][q]
        a, b = np.where(S["unify_has1"][q] > 0, pf[p1], -1), np.where(S["unify_has2"][q] > 0, pf[p2], -1)
        ok[q], uM[q], ucov[q] = oracle.check_unify(S["K"], S["iK"], S["histR"], S["histT"], S["histXY"], S["trackSpan"], a, b, S["unify_M1"][q],
                                                   S["unify_M2"][q], float(S["sigma"]))
    out["unify_ok"], out["unify_M"], out["unify_cov"] = ok, uM, ucov
    out["featRef"], out["segPool"] = feature_refs(S)
    return out


def _classify_expectations(S):
    import oracle

    out = dict(S)
    M, cov, fl = S["M0"].copy(), S["cov0"].copy(), S["flags"].copy()
    newpt, sfn, pf, fstat = S["newPt"].copy(), S["staticFrameNum"].copy(), S["pointFeat"].copy(), S["featStatic"].copy()
    N = fstat.shape[1]
    s2m = np.ascontiguousarray(np.where(pf.T >= 0, np.arange(N, dtype=np.int32)[None, :], -1).astype(np.int32))
    oracle.map_points_classify(S["K"], S["iK"], S["histR"], S["histT"], S["histXY"], S["trackSpan"], fstat, pf, int(S["curFrame"]), M, cov, fl,
                               newpt, sfn, S["firstFrame"], float(S["pixelVar"]), featFrame=S["featFrame"], featFirst=S["featFirst"], slot2map=s2m)
    out.update(M_ref=M, cov_ref=cov, flags_ref=fl, newPt_ref=newpt, staticFrameNum_ref=sfn, hasFeature_ref=(pf >= 0).astype(np.uint8),
               featStatic_ref=fstat)
    return out


def _classify_ref_expectations(S):
    """the layout of classify_relink_golden.npz: the same features as references (slot2map / refStatic beside them)"""
    import oracle
    from tests.test_oracle_cpu import classify_relink_expect

    out = dict(S)
    pf = S["pointFeat"]
    N = S["featStatic"].shape[1]
    out["featRef"], out["segPool"] = feature_refs(S)
    out["slot2map"] = np.ascontiguousarray(np.where(pf.T >= 0, np.arange(N, dtype=np.int32)[None, :], -1).astype(np.int32))
    out["refStatic"] = np.ascontiguousarray(np.where(pf >= 0, S["featStatic"].T[np.maximum(pf, 0), np.arange(pf.shape[1])[None, :]], 1).astype(np.uint8))
    M, cov, fl = S["M0"].copy(), S["cov0"].copy(), S["flags"].copy()
    newpt, sfn, pf, fstat, rstat = S["newPt"].copy(), S["staticFrameNum"].copy(), pf.copy(), S["featStatic"].copy(), out["refStatic"].copy()
    ref, s2m = out["featRef"].copy(), out["slot2map"].copy()
    oracle.map_points_classify_ref(S["K"], S["iK"], S["histR"], S["histT"], S["histXY"], S["trackSpan"], fstat, pf, ref, out["segPool"], rstat,
                                   int(S["curFrame"]), M, cov, fl, newpt, sfn, S["firstFrame"], float(S["pixelVar"]), slot2map=s2m)
    has, dyn = classify_relink_expect(lambda k: out[k], pf, ref, fstat, rstat)
    out.update(M_ref=M, cov_ref=cov, flags_ref=fl, newPt_ref=newpt, staticFrameNum_ref=sfn, hasFeature_ref=has, featDyn_ref=dyn)
    return out


def _pack(scenes):
    out = {"n_scenes": np.int32(len(scenes))}
    for i, S in enumerate(scenes):
        out.update({f"s{i}_{k}": v for k, v in S.items()})
    return out


_cache = {}


def update_scenes():
    """the 14- and 16-camera scenes in the layout of update_points_golden.npz (+ featRef / segPool), expectations from the oracle;
    computed once and shared: callers leave the arrays unchanged"""
    if "update" not in _cache:
        _cache["update"] = _pack([_update_expectations(make_scene(nC, 100 + nC)) for nC in CAMERA_COUNTS])
    return _cache["update"]


def classify_scenes():
    """the same scenes in the layout of classify_golden.npz, expectations from the oracle"""
    if "classify" not in _cache:
        _cache["classify"] = _pack([_classify_expectations(make_scene(nC, 100 + nC)) for nC in CAMERA_COUNTS])
    return _cache["classify"]


def chain_lengths(G):
    """[nP][nCams] nodes of every point's chain in a scene (G: array name -> array), 0 where the camera holds no feature; the feature's
    own run of frames plus, over references, the segments linked behind it"""
    try:
        ref, pool = G("featRef"), G("segPool")
    except KeyError:
        ref = None
    if ref is not None:
        nP, nC = ref.shape[:2]
        n = np.where(ref[:, :, 0] >= 0, ref[:, :, 1] - ref[:, :, 2] + 1, 0)
        for p in range(nP):
            for c in range(nC):
                s = ref[p, c, 3] if ref[p, c, 0] >= 0 else -1
                while s >= 0:
                    n[p, c] += pool[c, s, 1] - pool[c, s, 2] + 1
                    s = pool[c, s, 3]
        return n
    pf, span = G("pointFeat"), G("trackSpan")
    N, nC = span.shape[1] // 2, pf.shape[1]
    cams, slot = np.arange(nC)[None, :], np.maximum(pf, 0)
    return np.where(pf >= 0, span[cams, N + slot] - span[cams, slot] + 1, 0)


def coverage(G):
    """what a scene offers the lane layouts: points with a feature in every camera, the longest chain, and the checkUnify pairs with
    4 * nCams candidate views (both points seen by every camera, every chain with a node behind its feature)"""
    L = chain_lengths(G)
    nC = L.shape[1]
    out = dict(full=int(((L > 0).sum(axis=1) == nC).sum()), longest=int(L.max()))
    try:
        pts, h1, h2 = G("unify_pts"), G("unify_has1"), G("unify_has2")
    except KeyError:
        return out
    views = [int(((h1[q] > 0) * (1 + (L[pts[q][0]] >= 2))).sum() + ((h2[q] > 0) * (1 + (L[pts[q][1]] >= 2))).sum()) for q in range(len(pts))]
    out["pairs_all_views"] = int((np.array(views) == 4 * nC).sum())
    return out


def classify_ref_scenes():
    """the same scenes in the layout of classify_relink_golden.npz (one run of frames per feature, nothing linked behind)"""
    if "classify_ref" not in _cache:
        _cache["classify_ref"] = _pack([_classify_ref_expectations(make_scene(nC, 100 + nC)) for nC in CAMERA_COUNTS])
    return _cache["classify_ref"]
