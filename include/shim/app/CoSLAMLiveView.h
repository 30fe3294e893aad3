// -*- C++ -*-
// include/shim/app/CoSLAMLiveView.h -- the last two steps of the reference's frame over cs_liveview (coslam_amd/csrc/liveview.hip):
// CoSLAM::storeDynamicPoints (src/app/SL_CoSLAM.cpp:1900-1911), CoSLAM::getNumDynamicStaticPoints (:1447-1471) and the display's
// getDynTracks (src/gui/GLScenePane.cpp:19-52), each body replaced by one call:
//
//     CoSLAMLiveView<Point3dId> live(numCams, curCap, dynCap);           // once; Point3dId(x, y, z, id) is LibVisualSLAM's
//     live.frame(stream, curFrame, mapCap, d_mapCount, d_pointFeat, d_mapFlags, d_mapPts, d_R, d_t, d_groups);   // per frame: enqueued, no wait
//     void CoSLAM::storeDynamicPoints() { live.storeDynamicPoints(m_dynPts); }
//     void CoSLAM::getNumDynamicStaticPoints() { live.numDynamicStaticPoints(m_nStatic, m_nDynamic, m_nStaticFeat, m_nDynamicFeat, numCams); }
//     getDynTracks(m_pSLAM->m_dynPts, dynTracks, m_nTrjLen)  ->  live.getDynTracks(stream, dynTracks, m_nTrjLen);
//
// Header-only and templated on the point type, which is not in the reference tree: anything constructible as P(x, y, z, id) does.
// Two differences to the reference: a point's id is its MAP INDEX, not a value derived from its address; the device keeps
// trailDepth frames of dynamic points where m_dynPts grows without bound, so a trail is at most trailDepth long.
#ifndef COSLAM_LIVE_VIEW_H
#define COSLAM_LIVE_VIEW_H

#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

#include "coslam_hip.h"

template <class P>
class CoSLAMLiveView {
public:
    // depth: snapshots the pinned ring holds; trailDepth: frames of dynamic points kept for the trails (150: the display's default m_nTrjLen,
    // src/gui/GLScenePane.h:26); every: publish every that many frames (1: m_dynPts gets every frame, as in the reference)
    CoSLAMLiveView(int nCams, int curCap, int dynCap, int depth = 8, int trailDepth = 150, int every = 1, int device = 0)
        : _nCams(nCams), _dynCap(dynCap), _stored(-1), _view(cs_liveview_create(device, nCams, curCap, dynCap, depth, trailDepth, every)) {
        if (!_view) throw std::runtime_error(std::string("CoSLAMLiveView: ") + cs_last_error());
    }
    ~CoSLAMLiveView() { cs_liveview_destroy(_view); }
    CoSLAMLiveView(const CoSLAMLiveView&) = delete;
    CoSLAMLiveView& operator=(const CoSLAMLiveView&) = delete;

    cs_liveview* handle() const { return _view; }

    // the frame's step: enqueued on the stream, never waits (cs_liveview_frame_dev)
    void frame(void* hip_stream, int frame, int nMap, const int* d_mapCount, const int* d_pointFeat, const unsigned char* d_mapFlags,
               const double* d_mapPts, const double* d_R, const double* d_t, const cs_camera_groups* d_groups = 0) {
        ok(cs_liveview_frame_dev(_view, hip_stream, frame, nMap, d_mapCount, d_pointFeat, d_mapFlags, d_mapPts, d_R, d_t, d_groups));
    }

    // storeDynamicPoints: appends the dynamic points of the newest snapshot that HAS LANDED -- once per snapshot, so a call that finds nothing
    // new appends nothing (the reference's one-camera early return, :1901-1902, included: such a rig never appends).  Never waits.  Returns
    // whether a list was appended.  The list is read off the snapshot's records (flags == CS_MAP_DYNAMIC, map order): it is the frame's
    // dynamic list as long as the current points fit under curCap.
    bool storeDynamicPoints(std::vector<std::vector<P> >& m_dynPts) {
        if (_nCams == 1) return false;
        const int f = cs_liveview_newest(_view);
        if (f < 0 || f <= _stored) return false;
        const cs_live_header* h = 0;
        const cs_live_point* p = 0;
        ok(cs_liveview_fetch(_view, f, &h, &p));
        std::vector<P> pts;
        for (int k = 0; k < h->nCur && (int)pts.size() < _dynCap; ++k)
            if (p[k].flags == CS_MAP_DYNAMIC) pts.push_back(P(p[k].M[0], p[k].M[1], p[k].M[2], (size_t)p[k].id));
        m_dynPts.push_back(pts);
        _stored = f;
        return true;
    }

    // getNumDynamicStaticPoints off the newest landed snapshot (:1450-1455's five members); false when no snapshot has landed yet
    bool numDynamicStaticPoints(int& nStatic, int& nDynamic, int* nStaticFeat, int* nDynamicFeat, int numCams) {
        const int f = cs_liveview_newest(_view);
        if (f < 0) return false;
        const cs_live_header* h = 0;
        const cs_live_point* p = 0;
        ok(cs_liveview_fetch(_view, f, &h, &p));
        nStatic = h->counts.nStatic, nDynamic = h->counts.nDynamic;
        for (int j = 0; j < numCams && j < 16; ++j) nStaticFeat[j] = h->counts.nStaticFeat[j], nDynamicFeat[j] = h->counts.nDynamicFeat[j];
        return true;
    }

    // getDynTracks over the device's ring (cs_liveview_trails): trails newest first, in ascending id order.  Waits for the stream.
    void getDynTracks(void* hip_stream, std::vector<std::vector<P> >& dynTracks, int trjLen) {
        dynTracks.clear();
        if (trjLen <= 0) return;
        int n = 0;
        std::vector<int> ids(_dynCap), lens(_dynCap);
        std::vector<double> pts((size_t)_dynCap * trjLen * 3);
        ok(cs_liveview_trails(_view, hip_stream, trjLen, _dynCap, &n, ids.data(), lens.data(), pts.data()));
        for (int q = 0; q < n && q < _dynCap; ++q) {
            std::vector<P> tr;
            for (int l = 0; l < lens[q]; ++l) {
                const double* m = &pts[((size_t)q * trjLen + l) * 3];
                tr.push_back(P(m[0], m[1], m[2], (size_t)ids[q]));
            }
            dynTracks.push_back(tr);
        }
    }

private:
    static void ok(int rc) {
        if (rc != CS_OK) throw std::runtime_error(std::string("CoSLAMLiveView: ") + cs_last_error());
    }
    int _nCams, _dynCap, _stored;
    cs_liveview* _view;
};

#endif  // COSLAM_LIVE_VIEW_H
