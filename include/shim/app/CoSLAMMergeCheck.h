// -*- C++ -*-
// include/shim/app/CoSLAMMergeCheck.h -- MergeCameraGroup::checkPossibleMergable (reference src/app/SL_MergeCameraGroup.cpp:56-177) over
// cs_merge_check (coslam_amd/csrc/merge.hip), the body replaced by one call:
//
//     CoSLAMMergeCheck merger(numCams, N, mapCap);                       // once
//     merger.setTables(d_mapCount, d_mapPts, d_mapFlags);                // the device's map tables
//     merger.setCamera(c, cam);                                          // cs_merge_cam: the hand-back's xy / state / slot2map, K, R, t (device)
//     merger.setImageSize(c, w, h);                                      // MergeCameraGroup::setImageSize (one size for the rig)
//     merger.setCurrentFrame(kf->f, d_groups);                           // setCurrentFrame: the key frame and its record of the groups (device)
//     int n = merger.checkPossibleMergable(10, 0.5, Param::maxDistRatio);   // CoSLAM::mergeCamGroups, src/app/SL_CoSLAM.cpp:1380
//     merger.m_mergeInfo[k].frame1 / cam1 / gid1 / frame2 / cam2 / gid2    // MergeInfo, k < m_nMergeInfo
//
// Header-only and synchronous: one launch, one wait.  The m_lastFrmGroupMerge + 130 hold-off of mergeCamGroups stays with the caller (nothing
// behind the gate is built here).
#ifndef COSLAM_MERGE_CHECK_H
#define COSLAM_MERGE_CHECK_H

#include <stdexcept>
#include <string>

#include "coslam_hip.h"

class CoSLAMMergeCheck {
public:
    typedef cs_merge_info MergeInfo;
    MergeInfo m_mergeInfo[256];
    int m_nMergeInfo;
    cs_merge_candidates record;   // the whole answer of the last call: the overlap tables and distances behind the list

    CoSLAMMergeCheck(int nCams, int N, int nMap, int device = 0, void* hip_stream = 0)
        : m_nMergeInfo(0), _nCams(nCams), _N(N), _nMap(nMap), _device(device), _stream(hip_stream), _frame(-1), _W(0), _H(0), _mapCount(0),
          _mapPts(0), _mapFlags(0), _groups(0) {
        if (nCams < 1 || nCams > 16) throw std::runtime_error("CoSLAMMergeCheck: 1..16 cameras");
        for (int c = 0; c < 16; ++c) _cams[c] = cs_merge_cam();
    }
    void setTables(const int* d_mapCount, const double* d_mapPts, const unsigned char* d_mapFlags) {
        _mapCount = d_mapCount, _mapPts = d_mapPts, _mapFlags = d_mapFlags;
    }
    void setCamera(int iCam, const cs_merge_cam& cam) { _cams[at(iCam)] = cam; }
    void setImageSize(int iCam, int w, int h) {
        at(iCam);
        if (_W && (w != _W || h != _H)) throw std::runtime_error("CoSLAMMergeCheck: one image size for the rig");
        _W = w, _H = h;
    }
    void setCurrentFrame(int frame, const cs_camera_groups* d_groups) { _frame = frame, _groups = d_groups; }

    int checkPossibleMergable(int minNum, double minAreaRatio, double maxCamDist, bool allPairs = false) {
        const int rc = cs_merge_check(_device, _stream, _nCams, _cams, _N, _nMap, _mapCount, _mapPts, _mapFlags, _W, _H, _groups, _frame, minNum,
                                      minAreaRatio, maxCamDist, allPairs ? 1 : 0, &record);
        if (rc != CS_OK) throw std::runtime_error(std::string("CoSLAMMergeCheck: ") + cs_last_error());
        m_nMergeInfo = record.nMergeInfo;
        for (int k = 0; k < m_nMergeInfo; ++k) m_mergeInfo[k] = record.info[k];
        return m_nMergeInfo;
    }

private:
    int at(int iCam) const {
        if (iCam < 0 || iCam >= _nCams) throw std::runtime_error("CoSLAMMergeCheck: camera out of range");
        return iCam;
    }
    int _nCams, _N, _nMap, _device;
    void* _stream;
    int _frame, _W, _H;
    const int* _mapCount;
    const double* _mapPts;
    const unsigned char* _mapFlags;
    const cs_camera_groups* _groups;
    cs_merge_cam _cams[16];
};

#endif  // COSLAM_MERGE_CHECK_H
