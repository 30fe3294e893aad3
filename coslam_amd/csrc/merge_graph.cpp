// merge_graph.cpp -- the key-frame pose graph of a camera-group merge as a host plan (no device work); behind it the host
// halves of 3.21 (cs_merge_matched_groups) and 3.22 (cs_merge_first_constrain).
//
// Replaces MergeCameraGroup::searchFirstKeyFrameForMerge (src/app/SL_MergeCameraGroup.cpp:884-906) and the topology of
// _constructGraphForKeyFrms (:907-1035) over host copies of the key frames' records: which key frame is held fixed, the
// node table (key frame, camera) frame-major over the cameras of both groups, and the edges in the reference's order --
// what cs_posegraph_create_scaled takes.  The edges' transforms are data movement around it: cs_posegraph_edges_dev for the
// plain ones, MergeInfo::R / t for the constraint edges.
//
// The search loop is restated as written (:888-901):
//   for (kf = current; kf && n <= nMaxKeyFrms && !found; kf = kf->prev) {
//       if (kf->f >= firstConstrain->f) continue;          // skipped WITHOUT counting
//       found = some group of kf holds both camId1 and camId2;
//       fixed = kf; n++;                                    // the frame that ends the search BECOMES the fixed frame
//   }
// so up to nMaxKeyFrms + 1 older frames are visited, and with no older frame at all the reference asserts (here: an error).
#include <cstring>
#include <vector>

#include "cs_common.h"

extern "C" int cs_merge_keygraph_plan(int nKeyFrames, const int* frames, const cs_camera_groups* groups, int nCamIds, const int* camIds,
                                      int firstConstrain, int camId1, int camId2, int nInfos, const int* infos, int nMaxKeyFrame,
                                      int* fixedKeyFrame, int nodeCap, int* nNodes, int* nodeKf, int* nodeCam, unsigned char* fixed,
                                      int edgeCap, int* nEdges, int* id1, int* id2, int* scaleId, int* nConstraintEdge) {
    if (fixedKeyFrame) *fixedKeyFrame = -1;
    if (nNodes) *nNodes = 0;
    if (nEdges) *nEdges = 0;
    if (nConstraintEdge) *nConstraintEdge = 0;
    if (nKeyFrames <= 0 || !frames || !groups || nCamIds <= 0 || nCamIds > 16 || !camIds || firstConstrain < 0 ||
        firstConstrain >= nKeyFrames || nInfos < 0 || (nInfos > 0 && !infos) || !fixedKeyFrame || !nNodes || !nEdges) {
        cs_set_error("cs_merge_keygraph_plan: bad argument");
        return CS_ERR_INVALID;
    }
    for (int k = 1; k < nKeyFrames; ++k)
        if (frames[k] <= frames[k - 1]) {
            cs_set_error("cs_merge_keygraph_plan: key frames must be given oldest first (frame %d behind %d)", frames[k], frames[k - 1]);
            return CS_ERR_INVALID;
        }
    bool inIds[16] = {};
    for (int i = 0; i < nCamIds; ++i) {
        if (camIds[i] < 0 || camIds[i] >= 16 || (i > 0 && camIds[i] <= camIds[i - 1])) {
            cs_set_error("cs_merge_keygraph_plan: camIds must be ascending camera ids below 16");
            return CS_ERR_INVALID;
        }
        inIds[camIds[i]] = true;
    }
    auto inGroup = [](const cs_camera_groups& r, int g, int cam) {
        for (int i = 0; i < r.num[g]; ++i)
            if (r.camIds[g][i] == cam) return true;
        return false;
    };
    // searchFirstKeyFrameForMerge
    const int firstF = frames[firstConstrain];
    int fx = -1, n = 0;
    bool found = false;
    for (int k = nKeyFrames - 1; k >= 0 && n <= nMaxKeyFrame && !found; --k) {
        if (frames[k] >= firstF) continue;
        for (int g = 0; g < groups[k].groupNum; ++g)
            if (inGroup(groups[k], g, camId1) && inGroup(groups[k], g, camId2)) {
                found = true;
                break;
            }
        fx = k;
        n++;
    }
    if (fx < 0) {
        cs_set_error("cs_merge_keygraph_plan: no key frame is older than the first-constrained one (frame %d): nothing to hold fixed", firstF);
        return CS_ERR_INVALID;
    }
    *fixedKeyFrame = fx;
    // _constructGraphForKeyFrms: nodes
    const int nK = nKeyFrames - fx, nN = nK * nCamIds;
    int camPos[16];
    for (int c = 0; c < 16; ++c) camPos[c] = -1;
    for (int i = 0; i < nCamIds; ++i) camPos[camIds[i]] = i;
    std::vector<int> e1, e2, es;
    for (int k = fx; k < nKeyFrames; ++k) {
        const int base = (k - fx) * nCamIds;
        const cs_camera_groups& r = groups[k];
        for (int g = 0; g < r.groupNum; ++g) {
            int cams[16], m = 0;
            for (int i = 0; i < r.num[g] && i < 16; ++i)
                if (r.camIds[g][i] >= 0 && r.camIds[g][i] < 16 && inIds[r.camIds[g][i]]) cams[m++] = r.camIds[g][i];
            if (m > 1 && frames[k] <= firstF) {
                for (int i = 1; i < m; ++i) e1.push_back(base + camPos[cams[i - 1]]), e2.push_back(base + camPos[cams[i]]), es.push_back(-1);
                if (m > 2) e1.push_back(base + camPos[cams[m - 1]]), e2.push_back(base + camPos[cams[0]]), es.push_back(-1);
            }
        }
        if (k != fx)
            for (int i = 0; i < nCamIds; ++i) e1.push_back(base - nCamIds + i), e2.push_back(base + i), es.push_back(-1);
    }
    auto nodeOf = [&](int frame, int cam) {
        if (cam < 0 || cam >= 16 || camPos[cam] < 0) return -1;
        for (int k = fx; k < nKeyFrames; ++k)
            if (frames[k] == frame) return (k - fx) * nCamIds + camPos[cam];
        return -1;
    };
    for (int i = 0; i < nInfos; ++i) {
        const int a = nodeOf(infos[4 * i], infos[4 * i + 1]), b = nodeOf(infos[4 * i + 2], infos[4 * i + 3]);
        if (a < 0 || b < 0 || a == b) {
            cs_set_error("cs_merge_keygraph_plan: merge info %d (frame %d cam %d -> frame %d cam %d) does not name two nodes of the graph", i,
                         infos[4 * i], infos[4 * i + 1], infos[4 * i + 2], infos[4 * i + 3]);
            return CS_ERR_INVALID;
        }
        e1.push_back(a), e2.push_back(b), es.push_back(0);
    }
    *nNodes = nN;
    *nEdges = (int)e1.size();
    if (nConstraintEdge) *nConstraintEdge = nInfos;
    if (nN > nodeCap || (int)e1.size() > edgeCap) {
        cs_set_error("cs_merge_keygraph_plan: %d nodes / %d edges do not fit the capacities %d / %d", nN, (int)e1.size(), nodeCap, edgeCap);
        return CS_ERR_INVALID;
    }
    if ((nN > 0 && (!nodeKf || !nodeCam || !fixed)) || (!e1.empty() && (!id1 || !id2 || !scaleId))) {
        cs_set_error("cs_merge_keygraph_plan: null output array");
        return CS_ERR_INVALID;
    }
    for (int i = 0; i < nN; ++i) {
        nodeKf[i] = fx + i / nCamIds;
        nodeCam[i] = camIds[i % nCamIds];
        fixed[i] = i < nCamIds ? 1 : 0;
    }
    if (!e1.empty()) {
        memcpy(id1, e1.data(), sizeof(int) * e1.size());
        memcpy(id2, e2.data(), sizeof(int) * e2.size());
        memcpy(scaleId, es.data(), sizeof(int) * es.size());
    }
    return CS_OK;
}

// ---- MergeCameraGroup::mergeMatchedGroups (src/app/SL_MergeCameraGroup.cpp:1117-1174) and the m_groupId loop behind it
// (src/app/SL_CoSLAM.cpp:1419-1424) over a host record.  Groups joined by a valid merge info become one: the connected components of the
// group graph (findConnectedComponents is un-vendored LibVisualSLAM; the order is this library's definition, DESIGN 5.1: components by
// ascending smallest member, members ascending), the cameras appended group by group in each old group's own order (:1141-1148).
// mergedGid: the first new group that holds camid1 or camid2 (:1162-1171); none: the reference asserts, here an error and the record is
// left as it was.  Entries behind the new counts are cleared as cs_camera_grouping_dev leaves them (-1 / 0).
extern "C" int cs_merge_matched_groups(cs_camera_groups* groups, int nInfo, const int* gid1, const int* gid2, int camid1, int camid2,
                                       int* groupId, int* mergedGid) {
    if (mergedGid) *mergedGid = -1;
    if (!groups || nInfo < 0 || (nInfo > 0 && (!gid1 || !gid2)) || !groupId || !mergedGid || groups->groupNum < 1 || groups->groupNum > 16) {
        cs_set_error("cs_merge_matched_groups: bad argument");
        return CS_ERR_INVALID;
    }
    const int nG = groups->groupNum;
    for (int g = 0; g < nG; ++g)
        if (groups->num[g] < 0 || groups->num[g] > 16) {
            cs_set_error("cs_merge_matched_groups: group %d holds %d cameras", g, groups->num[g]);
            return CS_ERR_INVALID;
        }
    bool A[16][16] = {};
    for (int i = 0; i < nInfo; ++i) {
        if (gid1[i] < 0 || gid1[i] >= nG || gid2[i] < 0 || gid2[i] >= nG) {
            cs_set_error("cs_merge_matched_groups: merge info %d names group %d / %d of %d", i, gid1[i], gid2[i], nG);
            return CS_ERR_INVALID;
        }
        A[gid1[i]][gid2[i]] = A[gid2[i]][gid1[i]] = true;
    }
    int comp[16], nComp = 0;
    for (int g = 0; g < nG; ++g) comp[g] = -1;
    for (int g = 0; g < nG; ++g) {   // ascending smallest member
        if (comp[g] >= 0) continue;
        int stack[16], top = 0;
        stack[top++] = g, comp[g] = nComp;
        while (top > 0) {
            const int a = stack[--top];
            for (int b = 0; b < nG; ++b)
                if (A[a][b] && comp[b] < 0) comp[b] = nComp, stack[top++] = b;
        }
        ++nComp;
    }
    cs_camera_groups out;
    memset(&out, 0xFF, sizeof(out));
    out.groupNum = nComp;
    for (int g = 0; g < 16; ++g) out.num[g] = 0;
    for (int k = 0; k < nComp; ++k)
        for (int g = 0; g < nG; ++g) {   // members ascending
            if (comp[g] != k) continue;
            for (int i = 0; i < groups->num[g]; ++i) {
                if (out.num[k] >= 16) {
                    cs_set_error("cs_merge_matched_groups: more than 16 cameras in the merged group %d", k);
                    return CS_ERR_INVALID;
                }
                out.camIds[k][out.num[k]++] = groups->camIds[g][i];
            }
        }
    int mg = -1;
    for (int k = 0; k < nComp && mg < 0; ++k)
        for (int i = 0; i < out.num[k]; ++i)
            if (out.camIds[k][i] == camid1 || out.camIds[k][i] == camid2) {
                mg = k;
                break;
            }
    if (mg < 0) {
        cs_set_error("cs_merge_matched_groups: neither camera %d nor camera %d is in a group", camid1, camid2);
        return CS_ERR_INVALID;
    }
    for (int c = 0; c < 16; ++c) groupId[c] = groups->groupId[c];   // (:1419-1424 writes the cameras of the groups only)
    for (int k = 0; k < nComp; ++k)
        for (int i = 0; i < out.num[k]; ++i) {
            const int c = out.camIds[k][i];
            if (c >= 0 && c < 16) groupId[c] = k;
        }
    for (int c = 0; c < 16; ++c) out.groupId[c] = groupId[c];
    *groups = out;
    *mergedGid = mg;
    return CS_OK;
}

// ---- MergeCameraGroup::buildIdMapForSelfKeyPoses(camIds, nSelfMotion = 2) (src/app/SL_MergeCameraGroup.cpp:512-555) over host arrays: which
// key frame is m_pFirstConstrainFrm, and the pose order of the merge's bundle adjustment.  The loop is restated as written:
//   min_kf = current; for c in camIds: for (kf = current->prev, nself = 0; kf && nself < 2; kf = kf->prev)
//       if (kf->pPose[c]->bSelfMotion) { if (min_kf->f >= kf->f) min_kf = kf; nself++; }
// With no self-motion key frame at all min_kf stays the current key frame and the reference's ind_to_order maps both halves of the order onto
// the second one; that is refused here.
extern "C" int cs_merge_first_constrain(int nKeyFrames, const int* frames, const unsigned char* selfMotion, int nCams, int nCamIds,
                                        const int* camIds, int* firstConstrain, int* orderFrame, int* orderCam) {
    if (firstConstrain) *firstConstrain = -1;
    if (nKeyFrames <= 0 || !frames || !selfMotion || nCams < 1 || nCams > 16 || nCamIds <= 0 || nCamIds > 16 || !camIds || !firstConstrain ||
        !orderFrame || !orderCam) {
        cs_set_error("cs_merge_first_constrain: bad argument");
        return CS_ERR_INVALID;
    }
    for (int k = 1; k < nKeyFrames; ++k)
        if (frames[k] <= frames[k - 1]) {
            cs_set_error("cs_merge_first_constrain: key frames must be given oldest first (frame %d behind %d)", frames[k], frames[k - 1]);
            return CS_ERR_INVALID;
        }
    for (int i = 0; i < nCamIds; ++i)
        if (camIds[i] < 0 || camIds[i] >= nCams || (i > 0 && camIds[i] <= camIds[i - 1])) {
            cs_set_error("cs_merge_first_constrain: camIds must be ascending camera ids below %d", nCams);
            return CS_ERR_INVALID;
        }
    int mn = nKeyFrames - 1;
    for (int i = 0; i < nCamIds; ++i) {
        const int c = camIds[i];
        int nself = 0;
        for (int k = nKeyFrames - 2; k >= 0 && nself < 2; --k)
            if (selfMotion[(size_t)k * nCams + c]) {
                if (frames[mn] >= frames[k]) mn = k;
                nself++;
            }
    }
    if (mn == nKeyFrames - 1) {
        cs_set_error("cs_merge_first_constrain: no camera of the two groups has a self-motion key frame behind frame %d: no first-constrained frame",
                     frames[nKeyFrames - 1]);
        return CS_ERR_INVALID;
    }
    *firstConstrain = mn;
    for (int i = 0; i < nCamIds; ++i) {
        orderFrame[i] = frames[nKeyFrames - 1], orderCam[i] = camIds[i];
        orderFrame[nCamIds + i] = frames[mn], orderCam[nCamIds + i] = camIds[i];
    }
    return CS_OK;
}

// ---- the choice of the camera pair: MergeCameraGroup::matchMergableCameras' loop (src/app/SL_MergeCameraGroup.cpp:325-414), DESIGN 3.24 ----
// Restated as it runs: the entries classified into a std::map keyed (gId1, gId2) (group pairs in ascending key order, each pair's entries in
// list order); nMinNCCMatchNum = 20 per group pair; `featMatches[k].num > nMinNCCMatchNum` reads the global success count k, while
// `nMinNCCMatchNum = featMatches[i].num` reads the index i inside the group pair's list (an unfilled Matching counts 0); maxk and the pair
// survive from one group pair to the next.  The reference's `m_mergeInfo[i].valid = false` on a short SURF match writes an entry nothing
// reads again before the list is rebuilt: not restated.  matched with maxk == -1 is where the reference's run is undefined: status -1.
#include <map>
#include <utility>
extern "C" int cs_merge_match_select(int nInfo, const cs_merge_info* info, const int* surfNum, const unsigned char* ematOk, const int* nccNum,
                                     const unsigned char* eligible, const int* groupSize, cs_merge_match_choice* out) {
    if (out) {
        memset(out, 0xFF, sizeof(*out));   // every field -1
        out->status = 0;
    }
    if (nInfo < 0 || nInfo > 256 || !out || (nInfo > 0 && (!info || !surfNum || !ematOk || !nccNum)) || !groupSize) {
        cs_set_error("cs_merge_match_select: bad arguments (%d entries of at most 256)", nInfo);
        return CS_ERR_INVALID;
    }
    std::map<std::pair<int, int>, std::vector<int>> byPair;
    for (int e = 0; e < nInfo; ++e) {
        const int g1 = info[e].gid1, g2 = info[e].gid2;
        if (g1 < 0 || g2 >= 16 || g1 >= g2) {   // the reference asserts gId1 < gId2
            cs_set_error("cs_merge_match_select: entry %d names the groups %d / %d", e, g1, g2);
            return CS_ERR_INVALID;
        }
        byPair[std::make_pair(g1, g2)].push_back(e);
    }
    int featNum[512];   // featMatches[].num: k < nInfo <= 256, i < nInfo
    memset(featNum, 0, sizeof(featNum));
    bool matched = false;
    int k = 0;
    for (const auto& gp : byPair) {
        int nMinNCCMatchNum = 20;
        const std::vector<int>& list = gp.second;
        for (size_t i = 0; i < list.size(); ++i) {
            const int e = list[i];
            if (surfNum[e] < 25) continue;
            if (!ematOk[e]) continue;
            featNum[k] = nccNum[e];
            matched = true;
            if (featNum[k] > nMinNCCMatchNum && (!eligible || eligible[e])) {
                nMinNCCMatchNum = featNum[i];
                out->maxk = k, out->entry = e;
                out->maxiCam = info[e].cam1, out->maxjCam = info[e].cam2;
                out->maxgId1 = gp.first.first, out->maxgId2 = gp.first.second;
            }
            ++k;
        }
    }
    if (!matched) return CS_OK;   // status 0
    if (out->maxk < 0) {
        out->status = -1;
        return CS_OK;
    }
    out->status = 1;
    if (groupSize[out->maxgId1] > groupSize[out->maxgId2]) {
        out->gid1 = out->maxgId1, out->gid2 = out->maxgId2, out->camid1 = out->maxiCam, out->camid2 = out->maxjCam;
    } else {
        out->gid1 = out->maxgId2, out->gid2 = out->maxgId1, out->camid1 = out->maxjCam, out->camid2 = out->maxiCam;
    }
    return CS_OK;
}
