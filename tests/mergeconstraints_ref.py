"""A plain Python restatement of MergeCameraGroup::genMergeInfoVer2 (reference src/app/SL_MergeCameraGroup.cpp:557-725) up to the solver call
and behind it, over the library's tables: what cs_merge_first_constrain, cs_merge_constraints_assemble_dev and cs_merge_info_dev compute
(DESIGN 3.22).  Python floats are IEEE binary64 and every expression below is written in the operation order of the reference's helpers
(oracle/ref_shim: project, dist2, mat33AB, getRigidTransFromTo), so the results are the same bits.

A scene S is a dict: nC, N, nMap, nF, frame0 (the history holds frames frame0 .. f2 = frame0 + nF - 1), key_frames (ascending, last = f2),
self_motion [nKey][nC], groups (list of camera-id lists, the current key frame's record), gId1, gId2, maxiCam, maxjCam, K [nC][9],
histR [nC][nF][9], histT [nC][nF][3], histXY [nC][nF][2N], M [nMap][3], state [nC][N], slot2map [nC][N], featRef [nMap][nC][4] {slot, frame,
first, seg}, segPool [nC][cap][4] {slot, last, first, next}, matches [K][2] (slot in maxiCam, slot in maxjCam)."""
import math

VERDICT_MERGE, VERDICT_REJECT, VERDICT_FEW = 1, 0, -1
VIEW_FROM_M2, VIEW_DETACHED, VIEW_PREV, VIEW_PREV_DETACHED = 1, 2, 4, 8   # flags of a merge-list entry


def cam_ids_in_both_groups(groups, gId1, gId2):
    """getCamIdsInBothGroups: ascending"""
    return sorted(set(int(c) for c in groups[gId1]) | set(int(c) for c in groups[gId2]))


def first_constrain(key_frames, self_motion, cam_ids, n_self_motion=2):
    """buildIdMapForSelfKeyPoses -> (index of m_pFirstConstrainFrm, [(frame, cam)] in pose order), or None where no camera has a
    self-motion key frame behind the current one (the reference degenerates there; the library refuses)"""
    nk = len(key_frames)
    mn = nk - 1
    for c in cam_ids:
        nself, k = 0, nk - 2
        while k >= 0 and nself < n_self_motion:
            if self_motion[k][c]:
                if key_frames[mn] >= key_frames[k]:
                    mn = k
                nself += 1
            k -= 1
    if mn == nk - 1:
        return None
    return mn, [(int(key_frames[nk - 1]), c) for c in cam_ids] + [(int(key_frames[mn]), c) for c in cam_ids]


def project(K, R, t, M):
    X = R[0] * M[0] + R[1] * M[1] + R[2] * M[2] + t[0]
    Y = R[3] * M[0] + R[4] * M[1] + R[5] * M[2] + t[1]
    Z = R[6] * M[0] + R[7] * M[1] + R[8] * M[2] + t[2]
    u = K[0] * X + K[1] * Y + K[2] * Z
    v = K[3] * X + K[4] * Y + K[5] * Z
    w = K[6] * X + K[7] * Y + K[8] * Z
    return u / w, v / w


def dist2(a, b):
    return math.sqrt((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]))


def rigid_trans_from_to(R1, t1, R2, t2):
    """getRigidTransFromTo: R = R2 R1^T, t = t2 - R t1"""
    R1t = [R1[3 * j + i] for i in range(3) for j in range(3)]
    R = [R2[3 * i] * R1t[j] + R2[3 * i + 1] * R1t[3 + j] + R2[3 * i + 2] * R1t[6 + j] for i in range(3) for j in range(3)]
    t = [t2[r] - (R[3 * r] * t1[0] + R[3 * r + 1] * t1[1] + R[3 * r + 2] * t1[2]) for r in range(3)]
    return R, t


def find_prev(S, c, ref, f1, hop_cap):
    """the node of frame f1 on the chain behind the view {slot, frame, first, seg} of camera c: its slot, or -1.  The walk ends at the first
    run whose newest frame is older than f1, after hop_cap segments, or at a segment the pool does not hold."""
    slot, frame, first, seg = (int(v) for v in ref)
    hi, lo, hops = frame - 1, first, 0
    pool = S["segPool"][c]
    while True:
        if hi < f1:
            return -1
        if lo <= f1:
            return slot if 0 <= slot < S["N"] else -1
        if seg < 0 or seg >= len(pool) or hops >= hop_cap:
            return -1
        slot, hi, lo, seg = (int(v) for v in pool[seg])
        hops += 1


def assemble(S, f1, hop_cap=1 << 30, thres=500.0, detail=None):
    """-> dict(verdict, avgErr, cam_ids, order, nMergedTracks, nUnmerged, nPrevViews, skipped, views, Ks, Rs, Ts, pts, pointMap, obs_ptr, obs_cam,
    obs_xy).  views: the merge list, one [track, cam, slot, point, from, flags, prevSlot] per view of a merged track in track and view order."""
    nC, N, nMap, frame0 = S["nC"], S["N"], S["nMap"], S["frame0"]
    f2 = frame0 + S["nF"] - 1
    cam_ids = cam_ids_in_both_groups(S["groups"], S["gId1"], S["gId2"])
    order = [(f2, c) for c in cam_ids] + [(f1, c) for c in cam_ids]
    ind_to_order = {fc: i for i, fc in enumerate(order)}
    ref, state, s2m = S["featRef"], S["state"], S["slot2map"]
    out = dict(verdict=VERDICT_FEW, avgErr=0.0, cam_ids=cam_ids, order=order, nMergedTracks=0, nUnmerged=0, nPrevViews=0, skipped=0, views=[],
               Ks=[], Rs=[], Ts=[], pts=[], pointMap=[], obs_ptr=[0], obs_cam=[], obs_xy=[])
    pix = lambda c, f, s: (float(S["histXY"][c][f - frame0][s]), float(S["histXY"][c][f - frame0][N + s]))  # noqa: E731

    def cur_ref(m, c):
        r = ref[m][c]
        return 0 <= int(r[0]) < N and int(r[1]) == f2

    # 1. getCorresFeatPtsAndMapPts: every track from the state as given
    tracks = []   # [m1, [[cam, slot, from, first, seg], ...]]
    iC, jC = S["maxiCam"], S["maxjCam"]
    for a, b in S["matches"]:
        a, b = int(a), int(b)
        if not (0 <= a < N and 0 <= b < N and int(state[iC][a]) in (0, 1) and int(state[jC][b]) in (0, 1)):
            out["skipped"] += 1
            continue
        m1, m2 = int(s2m[iC][a]), int(s2m[jC][b])
        if not (0 <= m1 < nMap and 0 <= m2 < nMap):
            out["skipped"] += 1
            continue
        tk = []
        for c in cam_ids:
            for m in (m1, m2):
                if cur_ref(m, c):
                    r = ref[m][c]
                    tk.append([c, int(r[0]), m, int(r[2]), int(r[3])])
        tracks.append([m1, tk])
    nT = out["nMergedTracks"] = len(tracks)
    # 2. checkMergeMapPoints
    errs = []
    for m1, tk in tracks:
        Mp = [float(v) for v in S["M"][m1]]
        for c, s, _, _, _ in tk:
            i2 = f2 - frame0
            errs.append(dist2(project([float(v) for v in S["K"][c]], [float(v) for v in S["histR"][c][i2]], [float(v) for v in S["histT"][c][i2]], Mp),
                              pix(c, f2, s)))
    if nT == 0 or len(errs) < 3:
        return out
    top = sorted(errs, reverse=True)[:3]
    out["avgErr"] = ((top[0] + top[1]) + top[2]) / 3
    if out["avgErr"] > thres:
        out["verdict"] = VERDICT_REJECT
        return out
    out["verdict"] = VERDICT_MERGE
    # 3. mergeMapPoints, emitted: the state the later steps see
    slot_point = {}
    for m1, tk in tracks:
        for c, s, _, _, _ in tk:
            slot_point[(c, s)] = m1
    m1s = set(m1 for m1, _ in tracks)
    # 4. getUnMergedFeatureTracks
    cand = []
    for c in cam_ids:
        for s in range(N):
            if int(state[c][s]) not in (0, 1):
                continue
            q = slot_point.get((c, s), int(s2m[c][s]))
            if 0 <= q < nMap and q not in m1s:
                cand.append(q)
    vis = [sum(1 for c in range(nC) if cur_ref(q, c)) for q in cand]
    ranked = sorted(range(len(cand)), key=lambda i: -vis[i])   # stable
    max_num = 20 * nT
    for i in ranked:
        q = cand[i]
        tk = [[c, int(ref[q][c][0]), q, int(ref[q][c][2]), int(ref[q][c][3])] for c in cam_ids if cur_ref(q, c)]
        if len(tk) >= 1 and out["nUnmerged"] < max_num:
            tracks.append([q, tk])
            out["nUnmerged"] += 1
    if detail is not None:
        detail.update(n_candidates=len(cand), cand=cand, vis=vis)
    # 5. getCorresFeatPtsInPrevSelfKeyPoses
    prev = []
    for _, tk in tracks:
        pv = []
        for c, s, m, first, seg in tk:
            ps = find_prev(S, c, (s, f2, first, seg), f1, hop_cap)
            pv.append(ps)
            out["nPrevViews"] += ps >= 0
        prev.append(pv)
    # 6. the problem
    flags = {}
    kept = [t for t in range(len(tracks)) if len(tracks[t][1]) + sum(p >= 0 for p in prev[t]) > 1]
    if detail is not None:
        detail.update(dropped_tracks=len(tracks) - len(kept), tracks=tracks, prev=prev)
    for t in reversed(kept):
        m, tk = tracks[t]
        seen = set()
        for v, (c, s, _, _, _) in enumerate(tk):
            if (f2, c) in seen:
                flags[(t, v)] = flags.get((t, v), 0) | VIEW_DETACHED
                continue
            seen.add((f2, c))
            out["obs_cam"].append(ind_to_order[(f2, c)])
            out["obs_xy"].append(pix(c, f2, s))
        for v, (c, s, _, _, _) in enumerate(tk):
            if prev[t][v] < 0:
                continue
            if (f1, c) in seen:
                flags[(t, v)] = flags.get((t, v), 0) | VIEW_PREV_DETACHED
                continue
            seen.add((f1, c))
            out["obs_cam"].append(ind_to_order[(f1, c)])
            out["obs_xy"].append(pix(c, f1, prev[t][v]))
        out["pts"].append([float(v) for v in S["M"][m]])
        out["pointMap"].append(m)
        out["obs_ptr"].append(len(out["obs_cam"]))
    for t in range(nT):
        m1, tk = tracks[t]
        for v, (c, s, m, _, _) in enumerate(tk):
            fl = flags.get((t, v), 0) | (VIEW_FROM_M2 if m != m1 else 0) | (VIEW_PREV if prev[t][v] >= 0 else 0)
            out["views"].append([t, c, s, m1, m, fl, prev[t][v]])
    for f, c in order:
        out["Ks"].append([float(v) for v in S["K"][c]])
        out["Rs"].append([float(v) for v in S["histR"][c][f - frame0]])
        out["Ts"].append([float(v) for v in S["histT"][c][f - frame0]])
    return out


def merge_infos(S, Rs, Ts, order):
    """:681-722 -> ([frame1, cam1, gid1, frame2, cam2, gid2] per info, R [n][9], t [n][3])"""
    g1, g2 = S["gId1"], S["gId2"]
    f2, f1 = order[0][0], order[-1][0]
    ind = {fc: i for i, fc in enumerate(order)}
    cam_ids = [c for f, c in order[:len(order) // 2]]
    ints, R, t = [], [], []

    def add(fa, ca, ga, fb, cb, gb):
        p, q = ind[(fa, ca)], ind[(fb, cb)]
        r, tt = rigid_trans_from_to(Rs[p], Ts[p], Rs[q], Ts[q])
        ints.append([fa, ca, ga, fb, cb, gb])
        R.append(r)
        t.append(tt)

    for c2 in S["groups"][g2]:
        add(f2, int(S["groups"][g1][0]), g1, f2, int(c2), g2)
    for c1 in S["groups"][g1][1:]:
        add(f2, int(c1), g1, f2, int(S["groups"][g2][0]), g2)
    for c in cam_ids:
        add(f2, c, -1, f1, c, -1)
    return ints, R, t


def apply_views(S, views, f1):
    """what mergeMapPoints and the duplicate marks of :631-634 leave behind, from the merge list: (cur_mpt [nC][N] -- the map point of every
    slot that is a feature of the current frame, -1 none --, pfeat [nMap][nC][2] {slot, frame} of every point's references, the detached
    nodes as a sorted list of (cam, frame, slot))"""
    nC, N, nMap = S["nC"], S["N"], S["nMap"]
    f2 = S["frame0"] + S["nF"] - 1
    cur = [[int(S["slot2map"][c][s]) if int(S["state"][c][s]) in (0, 1) else -1 for s in range(N)] for c in range(nC)]
    pfeat = [[[int(S["featRef"][m][c][0]), int(S["featRef"][m][c][1])] if int(S["featRef"][m][c][0]) >= 0 else [-1, -1] for c in range(nC)]
             for m in range(nMap)]
    det = set()
    for _, c, s, m1, _, _, _ in views:
        cur[c][s] = m1
        pfeat[m1][c] = [s, f2]
    for _, c, s, _, _, fl, ps in views:
        if fl & VIEW_DETACHED:
            cur[c][s] = -1
            det.add((c, f2, s))
        if fl & VIEW_PREV_DETACHED:
            det.add((c, f1, ps))
    return cur, pfeat, sorted(det)
