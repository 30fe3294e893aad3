// -*- C++ -*-
// include/shim/app/CoSLAMMergeFront.h -- MergeCameraGroup::matchSURFPoints and ::computeEMat (reference src/app/SL_MergeCameraGroup.cpp:
// 190-241, 314-319) over the cs_merge_front handle (coslam_amd/csrc/merge_front.hip):
//
//     CoSLAMMergeFront front(numCams, maxPts, dimDesc, maxHyp, stream);                // once
//     front.setK(c, K);                                                                // m_pCurKeyFrm->pPose[c]->K
//     int n = front.matchSURFPoints(iCam, jCam, surfPts1, surfPts2, dimDesc, desc1, desc2, matches);                  // :368
//     int m = front.computeEMat(iCam, jCam, surfPts1, surfPts2, matches, newMatches, E, nRansac, 2.0, minInlierNum);   // :376
//
// surfPts1 / surfPts2 are the reference's Mat_d (rows, data: [rows][2]), desc1 / desc2 its vector<float> of rows x dimDesc, matches /
// newMatches its Matching (num, operator[] -> idx1 / idx2, clear(), add(idx1, idx2, dist)).  matchSurf / estimateEMat / evaluateEMat are
// this library's definitions.  computeEMat returns inlierNum, or 0 below minInlierNum (newMatches is then left alone, as the
// reference leaves it); `result` holds the record of the last computeEMat, seeds() its getMatchedPts(newMatches, ...) rows.
// Header-only and synchronous: every call uploads its lists, runs one job and waits.  Needs the HIP runtime header (hipMalloc).
#ifndef COSLAM_MERGE_FRONT_H
#define COSLAM_MERGE_FRONT_H

#include <hip/hip_runtime_api.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "coslam_hip.h"

class CoSLAMMergeFront {
public:
    cs_merge_front_buffers buffers;
    cs_merge_front_result result;   // of the last computeEMat
    unsigned long long seed;        // of the sample generator

    CoSLAMMergeFront(int nCams, int maxPts, int dimDesc, int maxHyp, void* hip_stream = 0, int device = 0)
        : seed(0), _nCams(nCams), _maxPts(maxPts), _dim(dimDesc), _stream(hip_stream), _dPts(0), _dDesc(0) {
        if (nCams < 1 || nCams > 16) throw std::runtime_error("CoSLAMMergeFront: 1..16 cameras");
        result = cs_merge_front_result();
        for (int c = 0; c < 16; ++c)
            for (int q = 0; q < 9; ++q) _K[c][q] = q % 4 == 0 ? 1.0 : 0.0;
        _mf = cs_merge_front_create(device, nCams, maxPts, dimDesc, 1, maxHyp);
        if (!_mf) fail();
        if (cs_merge_front_buffers_get(_mf, &buffers) != CS_OK) fail();
        if (hipMalloc((void**)&_dPts, 2 * (size_t)maxPts * 16) != hipSuccess || hipMalloc((void**)&_dDesc, 2 * (size_t)maxPts * dimDesc * 4) != hipSuccess)
            throw std::runtime_error("CoSLAMMergeFront: device memory for the point and descriptor lists");
    }
    ~CoSLAMMergeFront() {
        cs_merge_front_destroy(_mf);
        (void)hipFree(_dPts), (void)hipFree(_dDesc);
    }
    void setK(int iCam, const double K[9]) {
        for (int q = 0; q < 9; ++q) _K[at(iCam)][q] = K[q];
    }

    template <class MatT, class MatchingT>
    int matchSURFPoints(int iCam, int jCam, const MatT& pts1, const MatT& pts2, int dimDesc, const std::vector<float>& desc1,
                        const std::vector<float>& desc2, MatchingT& matches, double ratio = 0.8, double maxDist = 0.6) {
        cs_merge_front_cam cams[16];
        upload(iCam, jCam, pts1, pts2, cams);
        if (dimDesc != _dim || desc1.size() < (size_t)pts1.rows * _dim || desc2.size() < (size_t)pts2.rows * _dim)
            throw std::runtime_error("CoSLAMMergeFront: descriptor lists do not fit the point lists");
        float* d2 = _dDesc + (size_t)_maxPts * _dim;
        if ((pts1.rows && hipMemcpy(_dDesc, desc1.data(), (size_t)pts1.rows * _dim * 4, hipMemcpyHostToDevice) != hipSuccess) ||
            (pts2.rows && hipMemcpy(d2, desc2.data(), (size_t)pts2.rows * _dim * 4, hipMemcpyHostToDevice) != hipSuccess))
            throw std::runtime_error("CoSLAMMergeFront: descriptor upload");
        cams[iCam].desc = _dDesc, cams[jCam].desc = d2;
        cs_merge_front_job job = {iCam, jCam};
        if (cs_merge_front_match_dev(_mf, _stream, cams, 1, &job, ratio, maxDist) != CS_OK) fail();
        int n = 0;
        if (cs_merge_front_download(_mf, _stream, buffers.count, &n, sizeof(int)) != CS_OK) fail();
        std::vector<int> idx(2 * (size_t)(n > 0 ? n : 1));
        std::vector<float> dist(n > 0 ? n : 1);
        if (n > 0 && (cs_merge_front_download(_mf, _stream, buffers.matches, idx.data(), 8 * (size_t)n) != CS_OK ||
                      cs_merge_front_download(_mf, _stream, buffers.dist, dist.data(), 4 * (size_t)n) != CS_OK))
            fail();
        matches.clear();
        for (int k = 0; k < n; ++k) matches.add(idx[2 * k], idx[2 * k + 1], dist[k]);
        return n;
    }

    template <class MatT, class MatchingT>
    int computeEMat(int iCam, int jCam, const MatT& surfPts1, const MatT& surfPts2, const MatchingT& matches, MatchingT& newMatches, double E[9],
                    int nRansac, double maxEpiErr, int minInlierNum) {
        cs_merge_front_cam cams[16];
        upload(iCam, jCam, surfPts1, surfPts2, cams);
        if (matches.num > _maxPts) throw std::runtime_error("CoSLAMMergeFront: more matches than the handle holds");
        std::vector<int> idx(2 * (size_t)(matches.num > 0 ? matches.num : 1));
        for (int k = 0; k < matches.num; ++k) idx[2 * k] = matches[k].idx1, idx[2 * k + 1] = matches[k].idx2;
        const int* lists[1] = {idx.data()};
        const int nm = matches.num;
        cs_merge_front_job job = {iCam, jCam};
        if (cs_merge_front_from_matches_dev(_mf, _stream, cams, 1, &job, lists, &nm, nRansac, maxEpiErr, minInlierNum, seed) != CS_OK) fail();
        if (cs_merge_front_results(_mf, _stream, 1, &result) != CS_OK) fail();
        for (int q = 0; q < 9; ++q) E[q] = result.E[q];
        if (!result.ematOk) return 0;
        const int n = result.inlierNum;
        std::vector<int> in(2 * (size_t)(n > 0 ? n : 1));
        _seeds.assign(4 * (size_t)n, 0.0);
        if (n > 0 && (cs_merge_front_download(_mf, _stream, buffers.newMatches, in.data(), 8 * (size_t)n) != CS_OK ||
                      cs_merge_front_download(_mf, _stream, buffers.seeds, _seeds.data(), 32 * (size_t)n) != CS_OK))
            fail();
        newMatches.clear();
        for (int k = 0; k < n; ++k) newMatches.add(in[2 * k], in[2 * k + 1], 0);
        return n;
    }
    const std::vector<double>& seeds() const { return _seeds; }   // [inlierNum][4] = x1, y1, x2, y2 of the last successful computeEMat

private:
    int at(int iCam) const {
        if (iCam < 0 || iCam >= _nCams) throw std::runtime_error("CoSLAMMergeFront: camera out of range");
        return iCam;
    }
    template <class MatT>
    void upload(int iCam, int jCam, const MatT& pts1, const MatT& pts2, cs_merge_front_cam* cams) {
        at(iCam), at(jCam);
        if (iCam == jCam || pts1.rows > _maxPts || pts2.rows > _maxPts || pts1.rows < 0 || pts2.rows < 0)
            throw std::runtime_error("CoSLAMMergeFront: one camera twice, or more points than the handle holds");
        for (int c = 0; c < 16; ++c) cams[c].pts = 0, cams[c].desc = 0, cams[c].K = _K[c], cams[c].n = 0;
        double* p2 = _dPts + 2 * (size_t)_maxPts;
        if ((pts1.rows && hipMemcpy(_dPts, pts1.data, (size_t)pts1.rows * 16, hipMemcpyHostToDevice) != hipSuccess) ||
            (pts2.rows && hipMemcpy(p2, pts2.data, (size_t)pts2.rows * 16, hipMemcpyHostToDevice) != hipSuccess))
            throw std::runtime_error("CoSLAMMergeFront: point upload");
        cams[iCam].pts = _dPts, cams[iCam].n = pts1.rows, cams[jCam].pts = p2, cams[jCam].n = pts2.rows;
    }
    void fail() const { throw std::runtime_error(std::string("CoSLAMMergeFront: ") + cs_last_error()); }
    CoSLAMMergeFront(const CoSLAMMergeFront&);
    CoSLAMMergeFront& operator=(const CoSLAMMergeFront&);

    int _nCams, _maxPts, _dim;
    void* _stream;
    cs_merge_front* _mf;
    double* _dPts;
    float* _dDesc;
    double _K[16][9];
    std::vector<double> _seeds;
};

#endif
