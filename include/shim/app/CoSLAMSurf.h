// -*- C++ -*-
// include/shim/app/CoSLAMSurf.h -- ::detectSURFPoints(img, surfPts, surfDesc) as MergeCameraGroup::detectSURFPoints calls it (reference
// src/app/SL_MergeCameraGroup.cpp:308-313) over the cs_surf handle (coslam_amd/csrc/surf.hip):
//
//     int dimDesc = detectSURFPoints(m_pCurKeyFrm->pPose[iCam]->img, surfPts, surfDesc);                  // :311
//     int dimDesc = detectSURFPoints(surf, img, surfPts, surfDesc);                                       // a caller-held cs_surf*
//
// img is the reference's ImgG (rows, cols, data: rows x cols bytes), surfPts its Mat_d (resize(rows, cols), data: [n][2] = x, y), surfDesc
// its vector<float> of n x dimDesc.  The reference's SURF is external; the definition is this library's.  The first form keeps
// one handle per image size (CoSLAMSurfOptions: threshold, capacity, octaves, layers, dimension, upright, keep).  keep = CS_SURF_KEEP_STRONGEST: an
// image with more than maxPts maxima keeps those of the largest response instead of the first maxPts of the list.  Key points whose descriptor has
// zero norm (NaN coordinates) are left out of the lists.  Header-only and synchronous: upload, cs_surf_run_dev, counts, downloads.  Needs
// the HIP runtime header (hipMalloc).
#ifndef COSLAM_SURF_H
#define COSLAM_SURF_H

#include <hip/hip_runtime_api.h>

#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "coslam_hip.h"

struct CoSLAMSurfOptions {
    double hessianThreshold;
    int maxPts, nOctaves, nOctaveLayers, dimDesc, upright, device;
    void* stream;
    int keep;
    CoSLAMSurfOptions()
        : hessianThreshold(100.0), maxPts(4096), nOctaves(4), nOctaveLayers(2), dimDesc(64), upright(0), device(0), stream(0), keep(CS_SURF_KEEP_FIRST) {}
};
inline CoSLAMSurfOptions& coslamSurfOptions() {   // of the cached handles: set before the first call of an image size
    static CoSLAMSurfOptions o;
    return o;
}

// a caller-held single-camera handle
template <class ImgT, class MatT>
int detectSURFPoints(cs_surf* surf, const ImgT& img, MatT& surfPts, std::vector<float>& surfDesc, double hessianThreshold = 100.0, int upright = 0,
                     void* hip_stream = 0, int keepMode = CS_SURF_KEEP_FIRST) {
    struct Fail {
        static void now(const char* what) { throw std::runtime_error(std::string("detectSURFPoints: ") + what + ": " + cs_last_error()); }
    };
    cs_surf_buffers b;
    if (cs_surf_buffers_get(surf, &b) != CS_OK) Fail::now("buffers");
    if (cs_surf_keep_set(surf, keepMode) != CS_OK) Fail::now("keep");
    if (b.nCams != 1 || img.cols != b.W || img.rows != b.H) throw std::runtime_error("detectSURFPoints: the handle is of another image size, or not of one camera");
    unsigned char* d = 0;
    const size_t bytes = (size_t)b.W * b.H;
    if (hipMalloc((void**)&d, bytes) != hipSuccess || hipMemcpy(d, img.data, bytes, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        throw std::runtime_error("detectSURFPoints: image upload");
    }
    const unsigned char* table[1] = {d};
    int n = 0;
    const bool ok = cs_surf_run_dev(surf, hip_stream, table, b.W, hessianThreshold, upright) == CS_OK && cs_surf_counts(surf, hip_stream, &n, 0) == CS_OK;
    (void)hipFree(d);   // (cs_surf_counts waited)
    if (!ok) Fail::now("run");
    std::vector<double> pts(2 * (size_t)(n > 0 ? n : 1));
    std::vector<float> desc((size_t)(n > 0 ? n : 1) * b.dimDesc);
    if (n > 0 && (cs_surf_download(surf, hip_stream, b.pts, pts.data(), 16 * (size_t)n) != CS_OK ||
                  cs_surf_download(surf, hip_stream, b.desc, desc.data(), 4 * (size_t)n * b.dimDesc) != CS_OK))
        Fail::now("download");
    int keep = 0;
    for (int k = 0; k < n; ++k)
        if (pts[2 * k] == pts[2 * k]) {   // not NaN
            pts[2 * keep] = pts[2 * k], pts[2 * keep + 1] = pts[2 * k + 1];
            for (int q = 0; q < b.dimDesc; ++q) desc[(size_t)keep * b.dimDesc + q] = desc[(size_t)k * b.dimDesc + q];
            ++keep;
        }
    surfPts.resize(keep, 2);
    for (int k = 0; k < 2 * keep; ++k) surfPts.data[k] = pts[k];
    surfDesc.assign(desc.begin(), desc.begin() + (size_t)keep * b.dimDesc);
    return b.dimDesc;
}

// the reference's call: a handle cached per image size, made with coslamSurfOptions()
template <class ImgT, class MatT>
int detectSURFPoints(const ImgT& img, MatT& surfPts, std::vector<float>& surfDesc) {
    struct Cache {
        std::map<std::pair<int, int>, cs_surf*> m;
        ~Cache() {
            for (std::map<std::pair<int, int>, cs_surf*>::iterator it = m.begin(); it != m.end(); ++it) cs_surf_destroy(it->second);
        }
    };
    static Cache cache;
    const CoSLAMSurfOptions& o = coslamSurfOptions();
    cs_surf*& sf = cache.m[std::make_pair(img.cols, img.rows)];
    if (!sf) {
        sf = cs_surf_create(o.device, 1, img.cols, img.rows, o.maxPts, o.nOctaves, o.nOctaveLayers, o.dimDesc);
        if (!sf) throw std::runtime_error(std::string("detectSURFPoints: ") + cs_last_error());
    }
    return detectSURFPoints(sf, img, surfPts, surfDesc, o.hessianThreshold, o.upright, o.stream, o.keep);
}

#endif
