// -*- C++ -*-
// include/shim/app/CoSLAMMergeApply.h -- what CoSLAM::mergeCamGroups does between "matchMergableCameras() > 0" and
// currentMapPointsRegister (reference src/app/SL_CoSLAM.cpp:1405-1437) over cs_merge_keygraph_plan / cs_merge_apply_* /
// cs_merge_matched_groups / cs_recompute_map_points_keyfrms_dev (coslam_amd/csrc/merge_graph.cpp, merge_apply.hip), under the reference's
// names:
//
//     CoSLAMMergeApply mcg(numCams, h, stream);                              // h: the cs_track_history the loops live on
//     mcg.setKeyFrames(nKey, frames, groups, firstConstrain);                // the key frames oldest first, the current one last (host records)
//     mcg.setMergeInfo(nInfo, infos, gid1, gid2, d_infoR, d_infoT, camid1, camid2);   // the VALID MergeInfo: {frame1, cam1, frame2, cam2},
//                                                                            // their group ids, R / t in DEVICE memory (matchMergableCameras stays on the host)
//     mcg.searchFirstKeyFrameForMerge();                                     // + constructGraphForKeyFrms + constructGraphForAllFrms: the plan and the handle
//     mcg.recomputeKeyCamPoses();                                            // + recomputeAllCameraPoses: ONE enqueue, corrected poses into the history
//     m_mergedgid = mcg.mergeMatchedGroups(&m_groups, m_groupId);            // host
//     mcg.recomputeMapPoints(cams, d_featRef, nMap, d_mapCount, d_firstFrame, d_lastFrame, d_mapFlags, f_start, d_mapPts, d_mapCov,
//                            Const::PIXEL_ERR_VAR);                          // getMapPts(f_start, getLastFrame()) + recomputeMapPoints, guarded
//     mcg.wait();                                                            // the only wait; throws when a solve failed (nothing was written)
//
// Header-only.  getFirstFrame() / getLastFrame() are the fixed and the current key frame's numbers (f_start = max(getFirstFrame(),
// m_lastReleaseFrm) is the caller's, :1430-1434).
#ifndef COSLAM_MERGE_APPLY_H
#define COSLAM_MERGE_APPLY_H

#include <stdexcept>
#include <string>
#include <vector>

#include "coslam_hip.h"

class CoSLAMMergeApply {
public:
    CoSLAMMergeApply(int nCams, cs_track_history* h, void* hip_stream = 0, int device = 0)
        : _nCams(nCams), _device(device), _h(h), _stream(hip_stream), _a(0), _firstConstrain(0), _camid1(0), _camid2(0), _fixed(-1), _infoR(0),
          _infoT(0) {
        if (nCams < 1 || nCams > 16 || !h) throw std::runtime_error("CoSLAMMergeApply: 1..16 cameras and a history");
    }
    ~CoSLAMMergeApply() {
        if (_a) cs_merge_apply_destroy(_a);
    }
    void setKeyFrames(int nKey, const int* frames, const cs_camera_groups* groups, int firstConstrain) {
        _frames.assign(frames, frames + nKey), _groups.assign(groups, groups + nKey), _firstConstrain = firstConstrain;
    }
    void setMergeInfo(int nInfo, const int* infos /* [nInfo][4] */, const int* gid1, const int* gid2, const double* d_infoR, const double* d_infoT,
                      int camid1, int camid2) {
        _infos.assign(infos, infos + 4 * nInfo), _gid1.assign(gid1, gid1 + nInfo), _gid2.assign(gid2, gid2 + nInfo);
        _infoR = d_infoR, _infoT = d_infoT, _camid1 = camid1, _camid2 = camid2;
    }
    // searchFirstKeyFrameForMerge(nMaxKeyFrms) + constructGraphForKeyFrms + constructGraphForAllFrms
    void searchFirstKeyFrameForMerge(int nMaxKeyFrms = 100) {
        const int nKey = (int)_frames.size(), nInfo = (int)_gid1.size();
        // getCamIdsInBothGroups: the cameras of the groups the infos join, ascending
        const cs_camera_groups& cur = _groups.back();
        bool in[16] = {};
        for (int i = 0; i < nInfo; ++i)
            for (int side = 0; side < 2; ++side) {
                const int g = side ? _gid2[i] : _gid1[i];
                for (int k = 0; g >= 0 && g < cur.groupNum && k < cur.num[g]; ++k) in[cur.camIds[g][k]] = true;
            }
        std::vector<int> camIds;
        for (int c = 0; c < 16; ++c)
            if (in[c]) camIds.push_back(c);
        const int nodeCap = nKey * 16, edgeCap = 2 * nodeCap + nInfo + 1;
        std::vector<int> nodeKf(nodeCap), nodeCam(nodeCap), id1(edgeCap), id2(edgeCap), sid(edgeCap);
        std::vector<unsigned char> fixed(nodeCap);
        int nNodes = 0, nEdges = 0, nCon = 0;
        check(cs_merge_keygraph_plan(nKey, _frames.data(), _groups.data(), (int)camIds.size(), camIds.data(), _firstConstrain, _camid1, _camid2,
                                     nInfo, _infos.data(), nMaxKeyFrms, &_fixed, nodeCap, &nNodes, nodeKf.data(), nodeCam.data(), fixed.data(),
                                     edgeCap, &nEdges, id1.data(), id2.data(), sid.data(), &nCon));
        for (int i = 0; i < nNodes; ++i) nodeKf[i] -= _fixed;   // counted from the fixed key frame
        _keys.assign(_frames.begin() + _fixed, _frames.end());
        if (_a) cs_merge_apply_destroy(_a);
        _a = cs_merge_apply_create(_device, _nCams, (int)_keys.size(), _keys.data(), nNodes, nodeKf.data(), nodeCam.data(), fixed.data(), nEdges,
                                   id1.data(), id2.data(), sid.data());
        if (!_a) throw std::runtime_error(std::string("CoSLAMMergeApply: ") + cs_last_error());
    }
    int getFirstFrame() const { return _keys.empty() ? -1 : _keys.front(); }
    int getLastFrame() const { return _keys.empty() ? -1 : _keys.back(); }
    // recomputeKeyCamPoses + recomputeAllCameraPoses: one enqueue, the corrected poses land in the history (or nothing does)
    void recomputeKeyCamPoses() { check(cs_merge_apply_run_dev(need(), _h, _stream, _infoR, _infoT, 0)); }
    void recomputeAllCameraPoses() {}   // (done by recomputeKeyCamPoses: the two are one call here)
    int mergeMatchedGroups(cs_camera_groups* groups, int* groupId /* [16] */) {
        int mg = -1;
        check(cs_merge_matched_groups(groups, (int)_gid1.size(), _gid1.data(), _gid2.data(), _camid1, _camid2, groupId, &mg));
        return mg;
    }
    void recomputeMapPoints(const cs_poseupdate_cam* cams, const cs_feat_ref* d_featRef, int nMap, const int* d_mapCount, const int* d_firstFrame,
                            const int* d_lastFrame, const unsigned char* d_mapFlags, int f_start, double* d_mapPts, double* d_mapCov,
                            double pixel_var, int* d_counts = 0) {
        int nKey = 0;
        const int* d_keys = cs_merge_apply_key_frames(need(), &nKey);
        check(cs_recompute_map_points_keyfrms_dev(_h, _stream, cams, d_featRef, nMap, d_mapCount, d_firstFrame, d_lastFrame, d_mapFlags, f_start,
                                                  getLastFrame(), d_keys, nKey, d_mapPts, d_mapCov, pixel_var, 1, d_counts,
                                                  cs_merge_apply_guard(need())));
    }
    void wait() { check(cs_merge_apply_status(need(), _stream)); }

private:
    static void check(int rc) {
        if (rc != CS_OK) throw std::runtime_error(std::string("CoSLAMMergeApply: ") + cs_last_error());
    }
    cs_merge_apply* need() const {
        if (!_a) throw std::runtime_error("CoSLAMMergeApply: searchFirstKeyFrameForMerge first");
        return _a;
    }
    int _nCams, _device;
    cs_track_history* _h;
    void* _stream;
    cs_merge_apply* _a;
    int _firstConstrain, _camid1, _camid2, _fixed;
    const double *_infoR, *_infoT;
    std::vector<int> _frames, _keys, _infos, _gid1, _gid2;
    std::vector<cs_camera_groups> _groups;
};

#endif  // COSLAM_MERGE_APPLY_H
