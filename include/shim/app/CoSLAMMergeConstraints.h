// -*- C++ -*-
// include/shim/app/CoSLAMMergeConstraints.h -- MergeCameraGroup::genMergeInfoVer2 (reference src/app/SL_MergeCameraGroup.cpp:557-725) over
// cs_merge_first_constrain and the cs_merge_constraints handle (coslam_amd/csrc/merge_graph.cpp, merge_constraints.hip):
//
//     CoSLAMMergeConstraints merger(numCams, N, maxMatches, mapCap, history, stream);      // once
//     merger.setCamera(c, cam);                            // cs_merge_cam: the current key frame's xy / state / slot2map and K (device)
//     merger.setMap(d_featRef, d_mapPts);                  // the feature references [mapCap][numCams] and the map points
//     merger.setKeyFrames(nKey, frames, selfMotion);       // oldest first, the current key frame last; KeyPose::bSelfMotion [nKey][numCams]
//     merger.setCurrentFrame(h_groups, d_groups);          // the current key frame's record of the groups, host copy and device copy
//     merger.storeFeaturePoints(c, h_state);               // m_featPoints[c]: the slots with a feature (state 0 / 1), in slot order
//     if (merger.genMergeInfoVer2(gId1, gId2, maxiCam, maxjCam, featMatches[maxk])) ...    // SL_MergeCameraGroup.cpp:416
//     merger.m_mergeInfo[k] (frame1, camId1, groupId1, frame2, camId2, groupId2, valid, R, t), k < m_nMergeInfo; merger.firstConstrain
//     merger.buffers.infoR / infoT                         // the same R / t in device memory, what cs_merge_apply_run_dev takes
//
// featMatches is the reference's Matching (num, operator[] -> idx1 / idx2): indices into m_featPoints[maxiCam] / [maxjCam]; they are turned
// into slots here.  Header-only and synchronous (the solves wait).  false: checkMergeMapPoints said no, or there was nothing to judge; a
// failed solve throws and leaves m_nMergeInfo = 0.
//
//     merger.mergeMapPoints(d_pointFeat, d_featRef, d_refStatic, d_mapPts, true, d_counts);   // behind a true genMergeInfoVer2
//
// applies the merge list (mergeMapPoints :468-488, the duplicate marks of :631-634) and the solved points (:665-669) to the LIVE tables:
// cs_merge_constraints_apply_map_dev over the slot2map tables given to setCamera (they are written), one enqueue, no wait.
#ifndef COSLAM_MERGE_CONSTRAINTS_H
#define COSLAM_MERGE_CONSTRAINTS_H

#include <stdexcept>
#include <string>
#include <vector>

#include "coslam_hip.h"

class CoSLAMMergeConstraints {
public:
    struct MergeInfo {
        int frame1, camId1, groupId1, frame2, camId2, groupId2;
        bool valid;
        double R[9], t[3];
    };
    MergeInfo m_mergeInfo[48];
    int m_nMergeInfo;
    int firstConstrain;                    // index of m_pFirstConstrainFrm among the key frames (cs_merge_keygraph_plan's argument)
    std::vector<int> m_camIds;             // getCamIdsInBothGroups
    cs_merge_constraints_header header;    // of the last call
    cs_merge_constraints_buffers buffers;

    CoSLAMMergeConstraints(int nCams, int N, int maxMatches, int mapCap, const cs_track_history* history, void* hip_stream = 0, int device = 0)
        : m_nMergeInfo(0), firstConstrain(-1), _nCams(nCams), _N(N), _maxMatches(maxMatches), _mapCap(mapCap), _h(history), _stream(hip_stream),
          _featRef(0), _mapPts(0), _dGroups(0), _feat(16) {
        if (nCams < 1 || nCams > 16) throw std::runtime_error("CoSLAMMergeConstraints: 1..16 cameras");
        for (int c = 0; c < 16; ++c) _cams[c] = cs_merge_cam();
        _mc = cs_merge_constraints_create(device, nCams, N, maxMatches, mapCap);
        if (!_mc) fail();
        if (cs_merge_constraints_buffers_get(_mc, &buffers) != CS_OK) fail();
    }
    ~CoSLAMMergeConstraints() { cs_merge_constraints_destroy(_mc); }
    void setCamera(int iCam, const cs_merge_cam& cam) { _cams[at(iCam)] = cam; }
    void setMap(const cs_feat_ref* d_featRef, const double* d_mapPts) { _featRef = d_featRef, _mapPts = d_mapPts; }
    void setKeyFrames(int nKey, const int* frames, const unsigned char* selfMotion) {
        _frames.assign(frames, frames + nKey);
        _self.assign(selfMotion, selfMotion + (size_t)nKey * _nCams);
    }
    void setCurrentFrame(const cs_camera_groups& h_groups, const cs_camera_groups* d_groups) { _groups = h_groups, _dGroups = d_groups; }
    void storeFeaturePoints(int iCam, const int* h_state) {
        std::vector<int>& v = _feat[at(iCam)];
        v.clear();
        for (int s = 0; s < _N; ++s)
            if (h_state[s] == 0 || h_state[s] == 1) v.push_back(s);
    }

    template <class MatchingT> bool genMergeInfoVer2(int gId1, int gId2, int maxiCam, int maxjCam, const MatchingT& featMatches) {
        m_nMergeInfo = 0;
        if (gId1 < 0 || gId1 >= _groups.groupNum || gId2 < 0 || gId2 >= _groups.groupNum) throw std::runtime_error("CoSLAMMergeConstraints: group out of range");
        bool in[16] = {false};
        for (int q = 0; q < 2; ++q)
            for (int i = 0; i < _groups.num[q ? gId2 : gId1]; ++i) in[at(_groups.camIds[q ? gId2 : gId1][i])] = true;
        m_camIds.clear();
        for (int c = 0; c < 16; ++c)
            if (in[c]) m_camIds.push_back(c);
        int oF[32], oC[32];
        if (cs_merge_first_constrain((int)_frames.size(), _frames.data(), _self.data(), _nCams, (int)m_camIds.size(), m_camIds.data(), &firstConstrain, oF,
                                     oC) != CS_OK)
            fail();
        const std::vector<int>&fi = _feat[at(maxiCam)], &fj = _feat[at(maxjCam)];
        const int K = featMatches.num;
        if (K > _maxMatches) throw std::runtime_error("CoSLAMMergeConstraints: more matches than the handle was created for");
        std::vector<int> slots(2 * (size_t)(K > 0 ? K : 1));
        for (int k = 0; k < K; ++k) {   // list indices -> slots; an index outside the list stays a skip (-1)
            const int a = featMatches[k].idx1, b = featMatches[k].idx2;
            slots[2 * k] = a >= 0 && a < (int)fi.size() ? fi[a] : -1;
            slots[2 * k + 1] = b >= 0 && b < (int)fj.size() ? fj[b] : -1;
        }
        if (cs_merge_constraints_assemble(_mc, _h, _stream, _cams, _featRef, _mapCap, _mapPts, _dGroups, gId1, gId2, maxiCam, maxjCam,
                                              _frames[firstConstrain], _frames.back(), slots.data(), K) != CS_OK)
            fail();
        if (cs_merge_constraints_solve(_mc, _stream) != CS_OK) fail();                          // :646-647
        if (cs_merge_constraints_info_dev(_mc, _stream, _dGroups, gId1, gId2) != CS_OK) fail();  // :681-722
        if (cs_merge_constraints_header_get(_mc, _stream, &header) != CS_OK) fail();
        if (header.verdict != CS_MERGE_OK) return false;                                        // :575-576
        const int n = header.nInfo;
        std::vector<cs_merge_info> ints(n > 0 ? n : 1);
        std::vector<unsigned char> valid(n > 0 ? n : 1);
        std::vector<double> R(9 * (size_t)(n > 0 ? n : 1)), t(3 * (size_t)(n > 0 ? n : 1));
        if (n > 0 && (cs_merge_constraints_download(_mc, _stream, buffers.info, ints.data(), n * sizeof(cs_merge_info)) != CS_OK ||
                      cs_merge_constraints_download(_mc, _stream, buffers.infoValid, valid.data(), n) != CS_OK ||
                      cs_merge_constraints_download(_mc, _stream, buffers.infoR, R.data(), 72 * (size_t)n) != CS_OK ||
                      cs_merge_constraints_download(_mc, _stream, buffers.infoT, t.data(), 24 * (size_t)n) != CS_OK))
            fail();
        for (int k = 0; k < n; ++k) {   // addMergeInfo
            MergeInfo& mi = m_mergeInfo[k];
            mi.frame1 = ints[k].frame1, mi.camId1 = ints[k].cam1, mi.groupId1 = ints[k].gid1;
            mi.frame2 = ints[k].frame2, mi.camId2 = ints[k].cam2, mi.groupId2 = ints[k].gid2;
            mi.valid = valid[k] != 0;
            for (int q = 0; q < 9; ++q) mi.R[q] = R[9 * k + q];
            for (int q = 0; q < 3; ++q) mi.t[q] = t[3 * k + q];
        }
        m_nMergeInfo = n;
        return true;
    }

    // mergeMapPoints + `fp->mpt = 0` + the write of the solved coordinates into MapPoint::M, on the device; enqueues only.  The verdict is
    // read on the device: behind anything but CS_MERGE_OK nothing is written.  d_pointFeat / d_refStatic / d_mapPts / d_counts [6] may be 0.
    void mergeMapPoints(int* d_pointFeat, cs_feat_ref* d_featRef, unsigned char* d_refStatic, double* d_mapPts, bool applyPoints = true,
                        int* d_counts = 0) {
        int* s2m[16];
        for (int c = 0; c < 16; ++c) s2m[c] = c < _nCams ? const_cast<int*>(_cams[c].slot2map) : 0;
        if (cs_merge_constraints_apply_map_dev(_mc, _stream, s2m, d_pointFeat, d_featRef, d_refStatic, _mapCap, d_mapPts, applyPoints ? 1 : 0,
                                               d_counts) != CS_OK)
            fail();
    }

private:
    int at(int iCam) const {
        if (iCam < 0 || iCam >= _nCams) throw std::runtime_error("CoSLAMMergeConstraints: camera out of range");
        return iCam;
    }
    void fail() const { throw std::runtime_error(std::string("CoSLAMMergeConstraints: ") + cs_last_error()); }
    int _nCams, _N, _maxMatches, _mapCap;
    const cs_track_history* _h;
    void* _stream;
    const cs_feat_ref* _featRef;
    const double* _mapPts;
    const cs_camera_groups* _dGroups;
    cs_merge_constraints* _mc;
    cs_camera_groups _groups;
    cs_merge_cam _cams[16];
    std::vector<int> _frames;
    std::vector<unsigned char> _self;
    std::vector<std::vector<int> > _feat;
};

#endif  // COSLAM_MERGE_CONSTRAINTS_H
