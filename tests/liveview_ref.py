"""Restatement, written from the reference's text, of the frame's last step: which map points are on curMapPts (CoSLAM::mapStateUpdate,
reference src/app/SL_CoSLAM.cpp:1182-1197, in this repository's terms), CoSLAM::getNumDynamicStaticPoints (:1447-1471),
CoSLAM::storeDynamicPoints (:1900-1911) and the display's getDynTracks (src/gui/GLScenePane.cpp:19-52).  numpy / pure Python, test
infrastructure only; the device side is coslam_amd/csrc/liveview.hip.

The reference's types are LibVisualSLAM's (MapPoint lists, Point3dId) and getDynTracks is GUI code, so nothing of it can be compiled into a
test driver: the evidence is this restatement.  Two differences are stated in DESIGN 3.18: an id here is the point's MAP INDEX
(the reference's is derived from an address), and the device keeps trailDepth frames of dynamic lists where m_dynPts grows without bound."""
import numpy as np

MAP_DYNAMIC, MAP_FALSE, MAP_UNCERTAIN = 1, 2, 4   # CS_MAP_* (include/coslam_hip.h)


def participating(pointFeat, mapCount=None):
    """the rows on curMapPts, ascending: a point stays on the list while some camera holds a feature of it in the current frame
    (mapStateUpdate removes it when lastFrame < curFrame, :1184-1186) -- whatever its type: a false point is only moved to falseMapPts when it
    is removed (:1187-1188).  pointFeat [nMap][nCams]: the feature's slot in THIS frame or < 0; rows at or behind mapCount are no map points."""
    pf = np.asarray(pointFeat)
    n = pf.shape[0] if mapCount is None else max(0, min(int(mapCount), pf.shape[0]))
    return [r for r in range(n) if (pf[r] >= 0).any()]


def num_dynamic_static_points(pointFeat, mapFlags, mapCount=None):
    """getNumDynamicStaticPoints (:1447-1471).  isCertainStatic(): locally static and not uncertain -- no CS_MAP_* bit at all;
    isCertainDynamic(): locally dynamic and not uncertain -- CS_MAP_DYNAMIC and nothing else (a false point's type is TYPE_MAP_FALSE)."""
    pf = np.asarray(pointFeat)
    nC = pf.shape[1]
    nStatic = nDynamic = 0                                    # :1450-1451
    nStaticFeat, nDynamicFeat = [0] * nC, [0] * nC            # :1452-1455
    for r in participating(pf, mapCount):                     # :1456
        fl = 0 if mapFlags is None else int(mapFlags[r])
        if fl == 0:                                           # :1457-1458
            nStatic += 1
        elif fl == MAP_DYNAMIC:                               # :1459-1460
            nDynamic += 1
        for j in range(nC):                                   # :1462
            if pf[r, j] >= 0:                                 # :1463, pFeatures[j] of this frame
                if fl == 0:
                    nStaticFeat[j] += 1                       # :1464-1465
                elif fl == MAP_DYNAMIC:
                    nDynamicFeat[j] += 1                      # :1466-1467
    return dict(nStatic=nStatic, nDynamic=nDynamic, nStaticFeat=nStaticFeat, nDynamicFeat=nDynamicFeat)


def store_dynamic_points(pointFeat, mapFlags, mapPts, mapCount=None):
    """storeDynamicPoints (:1900-1911): the frame's list [(id, x, y, z), ...] in list (= map) order; one camera: nothing is stored -- the
    caller's m_dynPts gets an EMPTY list for the frame here, because the device ring advances every frame."""
    pf = np.asarray(pointFeat)
    if pf.shape[1] == 1:                                      # :1901-1902
        return []
    out = []
    for r in participating(pf, mapCount):                     # :1905
        if (0 if mapFlags is None else int(mapFlags[r])) == MAP_DYNAMIC:   # :1906
            out.append((r, float(mapPts[r][0]), float(mapPts[r][1]), float(mapPts[r][2])))   # :1907
    return out


def current_points(pointFeat, mapFlags, mapPts, mapCount=None):
    """the display's copy of curMapPts (GLScenePane::copyDispData, GLScenePane.cpp:55-58) as the snapshot's records:
    [(id, M, camMask, flags, numVisCam), ...] in map order"""
    pf = np.asarray(pointFeat)
    out = []
    for r in participating(pf, mapCount):
        mask = 0
        for j in range(pf.shape[1]):
            if pf[r, j] >= 0:
                mask |= 1 << j
        out.append((r, tuple(float(v) for v in mapPts[r]), mask, 0 if mapFlags is None else int(mapFlags[r]), bin(mask).count("1")))
    return out


def get_dyn_tracks(dynMapPts, trjLen):
    """getDynTracks (GLScenePane.cpp:19-52).  dynMapPts: the frames' lists, oldest first, of (id, x, y, z).  Returns
    [(id, [(x, y, z), ...] newest first), ...] in ascending id order (the iteration order of std::map<size_t, ...>, :48-51)."""
    tracks = {}
    if not dynMapPts:                                         # :24-25
        return []
    l = 0
    for pts in reversed(dynMapPts):                           # :28-30
        if not l < trjLen:
            break
        for (pid, x, y, z) in pts:
            if l == 0:                                        # :32-36: the newest frame's ids open the tracks
                tracks.setdefault(pid, []).append((x, y, z))
            elif pid in tracks:                               # :38-44: an older frame only extends them
                tracks[pid].append((x, y, z))
        l += 1
    return [(pid, tracks[pid]) for pid in sorted(tracks)]     # :48-51


def header_of(pointFeat, mapFlags, mapPts, mapCount, curCap, dynCap):
    """what a snapshot's header and lists must say for these tables: the counts, and both lists cut at their caps in map order"""
    cur = current_points(pointFeat, mapFlags, mapPts, mapCount)
    dyn = store_dynamic_points(pointFeat, mapFlags, mapPts, mapCount)
    out = num_dynamic_static_points(pointFeat, mapFlags, mapCount)
    out.update(cur=cur[:curCap], dyn=dyn[:dynCap], nCur=min(len(cur), curCap), nDyn=min(len(dyn), dynCap),
               curOverflow=max(0, len(cur) - curCap), dynOverflow=max(0, len(dyn) - dynCap))
    return out


# ---- planted tables of the GPU tests ---------------------------------------------------------------------------------------------------------
def planted(seed, nCams, nMap, mapCount, rows=(), density=0.4, dyn_share=0.3):
    """pointFeat / flags / points with the named rows taking part plus a seeded share of the rest (rows BEHIND mapCount included, so that
    rows that look as if they took part lie behind the count); every flag combination occurs; the points are arbitrary doubles"""
    rng = np.random.RandomState(seed)
    pf = np.full((nMap, nCams), -1, dtype=np.int32)
    take = rng.uniform(size=nMap) < density
    take[[r for r in rows if r < nMap]] = True
    for r in np.nonzero(take)[0]:
        cams = np.nonzero(rng.uniform(size=nCams) < 0.5)[0]
        if len(cams) == 0:
            cams = [int(rng.randint(nCams))]
        for c in cams:
            pf[r, c] = int(rng.randint(0, 4096))
    kinds = rng.uniform(size=nMap)
    flags = np.where(kinds < dyn_share, MAP_DYNAMIC, np.where(kinds < 0.7, 0, rng.randint(0, 8, size=nMap))).astype(np.uint8)
    pts = rng.normal(size=(nMap, 3)) * 10.0
    return dict(nCams=nCams, nMap=nMap, mapCount=mapCount, pointFeat=pf, mapFlags=flags, mapPts=np.ascontiguousarray(pts))


def trail_sequence(T=6):
    """the planted sequence of the trail tests and of tests/cxx/liveview_shim_test.cpp (which restates it): 2 cameras, 8 map rows, point r of
    frame f at (r + 0.25 f, 10 r - f, 0.5 r f); row 0 static throughout; A = row 1 dynamic throughout; B = row 3 dynamic, without a feature
    at frame 4, back at frame 5; C = row 4 dynamic up to frame 3 and static from frame 4; D = row 6 first seen (dynamic) at frame 5"""
    nC, nMap, out = 2, 8, []
    for f in range(T):
        pf = np.full((nMap, nC), -1, dtype=np.int32)
        fl = np.zeros(nMap, dtype=np.uint8)
        pts = np.array([[r + 0.25 * f, 10.0 * r - f, 0.5 * r * f] for r in range(nMap)], dtype=np.float64)
        seen = [(0, 0), (0, 1), (1, 0), (1, 1), (4, 0)] + ([(3, 1)] if f != 4 else []) + ([(6, 0), (6, 1)] if f == 5 else [])
        for r, c in seen:
            pf[r, c] = 10 * r + c
        fl[1] = fl[3] = fl[6] = MAP_DYNAMIC
        fl[4] = MAP_DYNAMIC if f <= 3 else 0
        out.append(dict(nCams=nC, nMap=nMap, mapCount=nMap, pointFeat=pf, mapFlags=fl, mapPts=pts))
    return out
