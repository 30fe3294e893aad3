"""A plain Python restatement of cs_merge_constraints_apply_map_dev: MergeCameraGroup::mergeMapPoints (reference
src/app/SL_MergeCameraGroup.cpp:468-488), the duplicate marks of :631-634 and the write of the solved coordinates (:665-669) over the
library's tables.  The loops are the reference's, sequential and in list order, so "the last one wins" is simply what a later iteration
leaves; only integers and copied doubles, so the results are the same bits.

A scene S is the dict of tests/mergeconstraints_ref.py with two optional tables: pointFeat [nMap][nC] (default: the reference's slot where its
frame is the current one, else -1) and refStatic [nMap][nC] (default: zeros)."""
import numpy as np

VIEW_DETACHED, VIEW_PREV_DETACHED = 2, 8


def point_feat(S):
    """this frame's feature of every point per camera: the reference's slot where its frame is f2"""
    f2 = S["frame0"] + S["nF"] - 1
    ref = np.asarray(S["featRef"], np.int32)
    return np.where((ref[:, :, 0] >= 0) & (ref[:, :, 1] == f2), ref[:, :, 0], -1).astype(np.int32)


def tables(S):
    """the four live tables and the map as int32 / uint8 / float64 arrays (copies)"""
    nMap, nC = S["nMap"], S["nC"]
    return dict(slot2map=np.array(S["slot2map"], np.int32), featRef=np.array(S["featRef"], np.int32).reshape(nMap, nC, 4),
                refStatic=np.array(S["refStatic"], np.uint8) if "refStatic" in S else np.zeros((nMap, nC), np.uint8),
                pointFeat=np.array(S["pointFeat"], np.int32) if "pointFeat" in S else point_feat(S), M=np.array(S["M"], np.float64).reshape(nMap, 3))


def apply_map(S, views, pointMap=None, solvedPts=None, f1=None):
    """views: the merge list, rows [track, cam, slot, point, from, flags, prevSlot]; pointMap [P] / solvedPts [P][3]: the solved problem, or
    None where no solve stands behind the list; f1: the first-constrained frame (names the marked nodes of the past frame).
    -> dict(slot2map, featRef, refStatic, pointFeat, M, counts [6], detached: sorted (cam, frame, slot) of the marked nodes)"""
    nC, N, nMap = S["nC"], S["N"], S["nMap"]
    T = tables(S)
    before_ref, before_stat = T["featRef"].copy(), T["refStatic"].copy()
    counts = [0] * 6
    ok = lambda c, s, m1, fr: 0 <= c < nC and 0 <= s < N and 0 <= m1 < nMap and 0 <= fr < nMap  # noqa: E731
    last_slot, last_row = {}, {}
    for i, (_, c, s, m1, fr, _, _) in enumerate(views):
        if not ok(c, s, m1, fr):
            counts[5] += 1
            continue
        counts[0] += 1
        T["slot2map"][c][s] = m1
        T["featRef"][m1][c] = before_ref[fr][c]          # the chain hangs on the reference: all four fields, as they stood before
        T["refStatic"][m1][c] = before_stat[fr][c]
        T["pointFeat"][m1][c] = s
        last_slot[(c, s)], last_row[(m1, c)] = i, i
    f2 = S["frame0"] + S["nF"] - 1
    det, nodes = set(), set()
    for i, (_, c, s, m1, fr, fl, ps) in enumerate(views):
        if not ok(c, s, m1, fr):
            continue
        if last_slot[(c, s)] != i or last_row[(m1, c)] != i:
            counts[5] += 1
        if last_row[(m1, c)] == i and fr != m1:
            counts[1] += 1
        if fl & VIEW_DETACHED:
            T["slot2map"][c][s] = -1
            det.add((c, s))
            nodes.add((c, f2, s))
        if fl & VIEW_PREV_DETACHED:
            counts[3] += 1
            nodes.add((c, f1, ps))
    counts[2] = len(det)
    if pointMap is not None:
        last = {}
        for i, m in enumerate(pointMap):
            m = int(m)
            if not 0 <= m < nMap:
                counts[5] += 1
                continue
            T["M"][m] = solvedPts[i]
            last[m] = i
        counts[4] = len(last)
        counts[5] += sum(1 for i, m in enumerate(pointMap) if 0 <= int(m) < nMap and last[int(m)] != i)
    T["counts"], T["detached"] = counts, sorted(nodes)
    return T


def walk_chain(S, c, ref):
    """every node (frame, slot) of the chain behind the reference {slot, frame, first, seg} of camera c, newest first"""
    slot, frame, first, seg = (int(v) for v in ref)
    if slot < 0:
        return []
    out = [(f, slot) for f in range(frame, first - 1, -1)]
    pool, hops = S["segPool"][c], 0
    while 0 <= seg < len(pool) and hops < len(pool):
        s, hi, lo, seg = (int(v) for v in pool[seg])
        out += [(f, s) for f in range(hi, lo - 1, -1)]
        hops += 1
    return out
