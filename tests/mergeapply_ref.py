"""numpy / plain-float restatement of what a camera-group merge does behind its pose correction:

  recompute_map_points_keyfrms   CoSLAM::getMapPts (reference src/app/SL_CoSLAM.cpp:1818-1851) + MergeCameraGroup::recomputeMapPoints
                                 (src/app/SL_MergeCameraGroup.cpp:1175-1183) = updateStaticPointPositionAtKeyFrms
                                 (src/slam/SL_CoSLAMHelper.cpp:395-451) per selected point
  merge_matched_groups           MergeCameraGroup::mergeMatchedGroups (:1117-1174) + the m_groupId loop (SL_CoSLAM.cpp:1419-1424)

Chains are held as the library holds them (include/coslam_hip.h, cs_feat_ref / cs_feat_seg): featRef [nMap][nC][4] = {slot, frame, first,
seg}, segPool [nC][cap][4] = {slot, last, first, next}.  The history is indexed by FRAME here: histR [nC][nF][9], histT [nC][nF][3],
histXY [nC][nF][2N], entry i = frame frame0 + i, the newest frame = frame0 + nF - 1.

The un-vendored LibVisualSLAM helpers (getCameraCenter, getAbsRadiansBetween, normPoint, triangulateMultiView, getTriangulateCovMat) are
the definitions of oracle/poseupdate_oracle.c (cam_center, cos_between, ne_add_view, sym33_cof, cov_add_view), restated operation for
operation in Python floats (IEEE binary64, no contraction), so the results can be compared bit for bit."""
import bisect
import math

import numpy as np


def cam_center(R, t):
    return [-((R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2]) for i in range(3)]


def cos_between(M, C0, C):
    a = [C0[0] - M[0], C0[1] - M[1], C0[2] - M[2]]
    b = [C[0] - M[0], C[1] - M[1], C[2] - M[2]]
    d = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    na = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    nb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]
    return d / math.sqrt(na * nb)


_I, _J = (0, 0, 0, 1, 1, 2), (0, 1, 2, 1, 2, 2)


def sym33_cof(N):
    c = [N[3] * N[5] - N[4] * N[4], N[2] * N[4] - N[1] * N[5], N[1] * N[4] - N[2] * N[3], N[0] * N[5] - N[2] * N[2], N[1] * N[2] - N[0] * N[4],
         N[0] * N[3] - N[1] * N[1]]
    return c, (N[0] * c[0] + N[1] * c[1]) + N[2] * c[2]


def ne_add_view(EN, Eg, iK, R, t, mx, my):
    w = (iK[6] * mx + iK[7] * my) + iK[8]
    x, y = ((iK[0] * mx + iK[1] * my) + iK[2]) / w, ((iK[3] * mx + iK[4] * my) + iK[5]) / w      # normPoint
    a0 = [R[0] - x * R[6], R[1] - x * R[7], R[2] - x * R[8]]
    a1 = [R[3] - y * R[6], R[4] - y * R[7], R[5] - y * R[8]]
    b0, b1 = x * t[2] - t[0], y * t[2] - t[1]
    for q in range(6):
        EN[q] = EN[q] + (a0[_I[q]] * a0[_J[q]] + a1[_I[q]] * a1[_J[q]])
    for q in range(3):
        Eg[q] = Eg[q] + (a0[q] * b0 + a1[q] * b1)


def cov_add_view(S, K, R, t, M):
    X = ((R[0] * M[0] + R[1] * M[1]) + R[2] * M[2]) + t[0]
    Y = ((R[3] * M[0] + R[4] * M[1]) + R[5] * M[2]) + t[1]
    Z = ((R[6] * M[0] + R[7] * M[1]) + R[8] * M[2]) + t[2]
    KR = [(K[3 * i] * R[j] + K[3 * i + 1] * R[3 + j]) + K[3 * i + 2] * R[6 + j] for i in range(3) for j in range(3)]
    u, v, w = (K[0] * X + K[1] * Y) + K[2] * Z, (K[3] * X + K[4] * Y) + K[5] * Z, (K[6] * X + K[7] * Y) + K[8] * Z
    ww = w * w
    Jm = [0.0] * 6
    for j in range(3):
        Jm[j] = (KR[j] * w - u * KR[6 + j]) / ww
        Jm[3 + j] = (KR[3 + j] * w - v * KR[6 + j]) / ww
    for q in range(6):
        S[q] = S[q] + (Jm[_I[q]] * Jm[_J[q]] + Jm[3 + _I[q]] * Jm[3 + _J[q]])


def triangulate(views, Ks, iKs, M, sigma, update_cov):
    """views: [(camera, R[9], t[3], mx, my)] in view order -> (M[3], cov[9] or None): triangulateMultiView + getTriangulateCovMat"""
    EN, Eg = [0.0] * 6, [0.0] * 3
    for c, R, t, mx, my in views:
        ne_add_view(EN, Eg, iKs[c], R, t, mx, my)
    cf, det = sym33_cof(EN)
    Mn = [((cf[0] * Eg[0] + cf[1] * Eg[1]) + cf[2] * Eg[2]) / det, ((cf[1] * Eg[0] + cf[3] * Eg[1]) + cf[4] * Eg[2]) / det,
          ((cf[2] * Eg[0] + cf[4] * Eg[1]) + cf[5] * Eg[2]) / det]
    if not update_cov:
        return Mn, None
    S = [0.0] * 6
    for c, R, t, _mx, _my in views:
        cov_add_view(S, Ks[c], R, t, Mn)
    cf, dS = sym33_cof(S)
    s2 = sigma * sigma
    c = [(cf[q] / dS) * s2 for q in range(6)]
    return Mn, [c[0], c[1], c[2], c[1], c[3], c[4], c[2], c[4], c[5]]


def walk_widest_key_node(c, ref, segPool, seg_cap, n_slots, keys, oldest, cur, centre_of, M, C0, angles=False):
    """:419-433 -- behind the head `ref` = (slot, frame, first, seg) of camera c: the key-frame node of the whole chain whose centre subtends
    the largest angle with C0 at M (strict >, from 0: the first of equals in the backward walk wins, an angle of 0 never).  Cosines are
    compared unless angles.  Returns dict(node=(slot, frame) or None, cut, nodes=[(frame, slot, cos)] in walk order, n_nonkey_wider)."""
    slot, hi, lo, seg = int(ref[0]), int(ref[1]) - 1, int(ref[2]), int(ref[3])
    best, best_cos, best_ang, nodes, cut, hops = None, 1.0, 0.0, [], False, 0
    while True:
        run_cut = lo < oldest                                        # the chain goes on behind the store's oldest frame
        flo, fhi = max(lo, oldest), min(hi, cur)
        if fhi >= flo:
            ka, kb = bisect.bisect_left(keys, flo), bisect.bisect_left(keys, fhi + 1)
            for k in range(kb - 1, ka - 1, -1):                      # fp = fp->preFrame, :423 if (fp->bKeyFrm)
                f = keys[k]
                cv = cos_between(M, C0, centre_of(c, f))
                nodes.append((f, slot, cv))
                if angles:
                    ang = abs(math.acos(max(-1.0, min(1.0, cv))))
                    if ang > best_ang:                               # :427
                        best_ang, best = ang, (slot, f)
                elif cv < best_cos:
                    best_cos, best = cv, (slot, f)
        if run_cut:
            cut = True
            break
        if seg < 0:
            break
        if seg >= seg_cap or hops >= seg_cap:                        # the hop guard: a corrupt pool cannot loop or read out of bounds
            cut = True
            break
        g = segPool[c][seg]
        hops += 1
        if g[0] < 0 or g[0] >= n_slots:
            cut = True
            break
        slot, hi, lo, seg = int(g[0]), int(g[1]), int(g[2]), int(g[3])
    return dict(node=best, cut=cut, nodes=nodes)


def recompute_map_points_keyfrms(Ks, iKs, histR, histT, histXY, frame0, featRef, segPool, map_count, firstFrame, lastFrame, flags, f_start,
                                 f_end, key_frames, M, cov, sigma, update_cov=True, seg_cap=None, angles=False, detail=None):
    """M [nMap][3] / cov [nMap][9] are updated IN PLACE; returns counts [4]: rows selected, re-triangulated, left with fewer than two views,
    walks cut.  detail (a dict or None) receives per selected row m: dict(views=[(camera, frame, slot)], walks={camera: walk record})."""
    nC, nF = histR.shape[0], histR.shape[1]
    N = histXY.shape[2] // 2
    cur, oldest = frame0 + nF - 1, frame0
    keys = [int(k) for k in key_frames]
    assert keys == sorted(set(keys))
    keyset = set(keys)
    seg_cap = segPool.shape[1] if seg_cap is None else seg_cap
    Kl, iKl = [[float(v) for v in np.asarray(k).reshape(9)] for k in Ks], [[float(v) for v in np.asarray(k).reshape(9)] for k in iKs]
    Rl, Tl = histR.reshape(nC, nF, 9).tolist(), histT.reshape(nC, nF, 3).tolist()
    cen = {}

    def centre_of(c, f):
        if (c, f) not in cen:
            cen[(c, f)] = cam_center(Rl[c][f - frame0], Tl[c][f - frame0])
        return cen[(c, f)]

    counts = [0, 0, 0, 0]
    n_rows = min(int(map_count), featRef.shape[0]) if map_count is not None else featRef.shape[0]
    for m in range(max(n_rows, 0)):
        if flags[m] != 0 or lastFrame[m] < f_start or firstFrame[m] > f_end:           # SL_CoSLAM.cpp:1827-1831 isCertainStatic
            continue
        counts[0] += 1
        Mm = [float(v) for v in M[m]]
        views, rec = [], dict(views=[], walks={})
        for c in range(nC):                                                            # :400
            s, f0 = int(featRef[m, c, 0]), int(featRef[m, c, 1])
            if s < 0 or s >= N or f0 < oldest or f0 > cur or f0 not in keyset:         # :402 fp && fp->bKeyFrm (a key frame the store holds)
                continue
            i0 = f0 - frame0
            views.append((c, Rl[c][i0], Tl[c][i0], float(histXY[c, i0, s]), float(histXY[c, i0, N + s])))   # :407-414
            rec["views"].append((c, f0, s))
            w = walk_widest_key_node(c, featRef[m, c], segPool, seg_cap, N, keys, oldest, cur, centre_of, Mm, centre_of(c, f0), angles)
            rec["walks"][c] = w
            counts[3] += 1 if w["cut"] else 0
            if w["node"] is not None:                                                  # :434-443
                bs, bf = w["node"]
                i1 = bf - frame0
                views.append((c, Rl[c][i1], Tl[c][i1], float(histXY[c, i1, bs]), float(histXY[c, i1, N + bs])))
                rec["views"].append((c, bf, bs))
        if detail is not None:
            detail[m] = rec
        if len(views) < 2:                                                             # :446
            counts[2] += 1
            continue
        counts[1] += 1
        Mn, cv = triangulate(views, Kl, iKl, Mm, sigma, update_cov)
        M[m] = Mn
        if update_cov:
            cov[m] = cv
    return counts


def merge_matched_groups(groups, gid1, gid2, camid1, camid2, group_id=None):
    """groups: [[camera, ...], ...] -> (new groups, groupId [16], mergedGid); None where the reference asserts.  Components by ascending
    smallest member, members ascending (this library's definition of findConnectedComponents' order), the cameras appended group by group
    in each old group's own order (:1141-1148)."""
    nG = len(groups)
    adj = [[False] * nG for _ in range(nG)]
    for a, b in zip(gid1, gid2):
        adj[a][b] = adj[b][a] = True
    comp, comps = [-1] * nG, []
    for g in range(nG):
        if comp[g] >= 0:
            continue
        comp[g], stack, members = len(comps), [g], []
        while stack:
            a = stack.pop()
            members.append(a)
            for b in range(nG):
                if adj[a][b] and comp[b] < 0:
                    comp[b] = len(comps)
                    stack.append(b)
        comps.append(sorted(members))
    out = [[c for g in members for c in groups[g]] for members in comps]
    mg = next((k for k, g in enumerate(out) if camid1 in g or camid2 in g), None)
    if mg is None:
        return None
    gid = [-1] * 16 if group_id is None else [int(v) for v in group_id]
    if group_id is None:
        for g, cams in enumerate(groups):
            for c in cams:
                gid[c] = g
    for k, cams in enumerate(out):
        for c in cams:
            gid[c] = k
    return out, gid, mg
