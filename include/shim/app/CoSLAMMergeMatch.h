// -*- C++ -*-
// include/shim/app/CoSLAMMergeMatch.h -- MergeCameraGroup::matchFeaturePointsNCC (reference src/app/SL_MergeCameraGroup.cpp:262-307) and the
// choice of the camera pair in matchMergableCameras (:320-421) over the cs_merge_match handle and cs_merge_match_select
// (coslam_amd/csrc/merge_match.hip, merge_graph.cpp):
//
//     CoSLAMMergeMatch matcher(numCams, N, maxSeeds, pairCap, maxMatches, stream);     // once
//     matcher.setCamera(c, cam);                          // cs_merge_match_cam: the current key frame's xy / state and the small image (device), K (host), imgScale
//     matcher.setSmallImageSize(Ws, Hs);                  // KeyPose::imgSmall: one size for the rig
//     matcher.storeFeaturePoints(c, h_state);             // m_featPoints[c]: the slots with a feature (state 0 / 1), in slot order
//     int n = matcher.matchFeaturePointsNCC(iCam, jCam, surfPts1, surfPts2, newMatches, E, featMatches[k], 20.0, 0.45, 150);   // :381-383
//     int n = matcher.matchFeaturePointsNCCFront(iCam, jCam, fb.results + k, fb.seeds + 4 * (size_t)fb.maxPts * k, fb.maxPts, featMatches[k], 20.0, 0.45, 150);
//                                                         // the same with E, the seed count and the seed rows read ON THE DEVICE from job k of a
//                                                         // cs_merge_front (fb: its cs_merge_front_buffers); 0 matches for a job the front gave up
//     matcher.matches_ptr()                               // the same matches as SLOT pairs in device memory: cs_merge_constraints_assemble_dev's d_matches
//     CoSLAMMergeMatch::select(...)                       // the loop's choice: cs_merge_match_select
//
// surfPts1 / surfPts2 are the reference's Mat_d (rows, data: [rows][2]) of SURF positions, newMatches its Matching of the E matrix' inliers
// (num, operator[] -> idx1 / idx2): getMatchedPts(newMatches, surfPts1, surfPts2) is done here.  featMatches is the reference's Matching
// (clear(), add(idx1, idx2, dist)): it receives LIST indices into m_featPoints[iCam] / [jCam] (the slots' ranks) in acceptance order with
// the NCC score.  SURF detection / matching and estimateEMat / evaluateEMat stay the caller's.  Header-only and synchronous: one wait.
// A job whose candidate list or matches overflowed the handle throws (the result would not be the reference's).
#ifndef COSLAM_MERGE_MATCH_H
#define COSLAM_MERGE_MATCH_H

#include <stdexcept>
#include <string>
#include <vector>

#include "coslam_hip.h"

class CoSLAMMergeMatch {
public:
    cs_merge_match_buffers buffers;
    cs_merge_match_count count;   // of the last call: matches, flags, candidates, rounds

    CoSLAMMergeMatch(int nCams, int N, int maxSeeds, int pairCap, int maxMatches, void* hip_stream = 0, int device = 0)
        : _nCams(nCams), _N(N), _Ws(0), _Hs(0), _stream(hip_stream), _feat(16), _rank(16) {
        if (nCams < 1 || nCams > 16) throw std::runtime_error("CoSLAMMergeMatch: 1..16 cameras");
        for (int c = 0; c < 16; ++c) _cams[c] = cs_merge_match_cam();
        count = cs_merge_match_count();
        _mm = cs_merge_match_create(device, nCams, N, 1, maxSeeds, pairCap, maxMatches);
        if (!_mm) fail();
        if (cs_merge_match_buffers_get(_mm, &buffers) != CS_OK) fail();
    }
    ~CoSLAMMergeMatch() { cs_merge_match_destroy(_mm); }
    void setCamera(int iCam, const cs_merge_match_cam& cam) { _cams[at(iCam)] = cam; }
    void setSmallImageSize(int Ws, int Hs) { _Ws = Ws, _Hs = Hs; }
    void storeFeaturePoints(int iCam, const int* h_state) {
        std::vector<int>&v = _feat[at(iCam)], &r = _rank[iCam];
        v.clear();
        r.assign(_N, -1);
        for (int s = 0; s < _N; ++s)
            if (h_state[s] == 0 || h_state[s] == 1) r[s] = (int)v.size(), v.push_back(s);
    }
    const int* matches_ptr() const { return buffers.matches; }   // job 0: [count.count][2] slot pairs

    template <class MatT, class SurfMatchingT, class MatchingT>
    int matchFeaturePointsNCC(int iCam, int jCam, const MatT& surfPts1, const MatT& surfPts2, const SurfMatchingT& surfMatches, const double E[9],
                              MatchingT& featMatches, double maxEpiErr, double minNcc, double maxDisp) {
        at(iCam), at(jCam);
        std::vector<double> seeds(4 * (size_t)(surfMatches.num > 0 ? surfMatches.num : 1));
        for (int k = 0; k < surfMatches.num; ++k) {   // getMatchedPts
            const int a = surfMatches[k].idx1, b = surfMatches[k].idx2;
            if (a < 0 || a >= surfPts1.rows || b < 0 || b >= surfPts2.rows) throw std::runtime_error("CoSLAMMergeMatch: SURF match outside the point lists");
            seeds[4 * k] = surfPts1.data[2 * a], seeds[4 * k + 1] = surfPts1.data[2 * a + 1];
            seeds[4 * k + 2] = surfPts2.data[2 * b], seeds[4 * k + 3] = surfPts2.data[2 * b + 1];
        }
        cs_merge_match_job job;
        job.iCam = iCam, job.jCam = jCam, job.nSeeds = surfMatches.num, job.seeds = seeds.data();
        for (int q = 0; q < 9; ++q) job.E[q] = E[q];
        if (cs_merge_match_run_dev(_mm, _stream, _cams, _Ws, _Hs, 1, &job, maxEpiErr, minNcc, maxDisp) != CS_OK) fail();
        return finish(iCam, jCam, featMatches);
    }

    // the job's E, seed count and seed rows from device memory (cs_merge_match_run_front_dev): d_result one cs_merge_front_result, d_seeds its
    // [seedRows][4] rows.  A job with fewer than minSurfNum SURF matches or without E is skipped: no matches, count.flags = CS_MERGE_MATCH_SKIPPED.
    template <class MatchingT>
    int matchFeaturePointsNCCFront(int iCam, int jCam, const cs_merge_front_result* d_result, const double* d_seeds, int seedRows,
                                   MatchingT& featMatches, double maxEpiErr, double minNcc, double maxDisp, int minSurfNum = 25) {
        cs_merge_front_job pair;
        pair.iCam = at(iCam), pair.jCam = at(jCam);
        if (cs_merge_match_run_front_dev(_mm, _stream, _cams, _Ws, _Hs, 1, &pair, d_result, d_seeds, seedRows, minSurfNum, maxEpiErr, minNcc, maxDisp) !=
            CS_OK)
            fail();
        return finish(iCam, jCam, featMatches);
    }

private:
    template <class MatchingT>
    int finish(int iCam, int jCam, MatchingT& featMatches) {
        if (cs_merge_match_counts(_mm, _stream, 1, &count) != CS_OK) fail();
        if (count.flags == CS_MERGE_MATCH_SKIPPED) {
            featMatches.clear();
            return 0;
        }
        if (count.flags) throw std::runtime_error("CoSLAMMergeMatch: the candidate list or the matches or the seed rows overflowed the handle (flags " + std::to_string(count.flags) + ")");
        const int n = count.count;
        std::vector<int> slots(2 * (size_t)(n > 0 ? n : 1));
        std::vector<double> score(n > 0 ? n : 1);
        if (n > 0 && (cs_merge_match_download(_mm, _stream, buffers.matches, slots.data(), 8 * (size_t)n) != CS_OK ||
                      cs_merge_match_download(_mm, _stream, buffers.scores, score.data(), 8 * (size_t)n) != CS_OK))
            fail();
        featMatches.clear();
        for (int k = 0; k < n; ++k) featMatches.add(_rank[iCam][slots[2 * k]], _rank[jCam][slots[2 * k + 1]], score[k]);   // slots -> list indices
        return n;
    }

public:
    // matchMergableCameras' loop over the gate's list (cs_merge_match_select): nccNum[e] = featMatches of entry e (0 where the entry was skipped)
    static cs_merge_match_choice select(int nInfo, const cs_merge_info* info, const int* surfNum, const unsigned char* ematOk, const int* nccNum,
                                        const cs_camera_groups& groups) {
        cs_merge_match_choice out;
        if (cs_merge_match_select(nInfo, info, surfNum, ematOk, nccNum, 0, groups.num, &out) != CS_OK)
            throw std::runtime_error(std::string("CoSLAMMergeMatch: ") + cs_last_error());
        return out;
    }

private:
    int at(int iCam) const {
        if (iCam < 0 || iCam >= _nCams) throw std::runtime_error("CoSLAMMergeMatch: camera out of range");
        return iCam;
    }
    void fail() const { throw std::runtime_error(std::string("CoSLAMMergeMatch: ") + cs_last_error()); }
    CoSLAMMergeMatch(const CoSLAMMergeMatch&);
    CoSLAMMergeMatch& operator=(const CoSLAMMergeMatch&);

    int _nCams, _N, _Ws, _Hs;
    void* _stream;
    cs_merge_match* _mm;
    cs_merge_match_cam _cams[16];
    std::vector<std::vector<int> > _feat, _rank;
};

#endif
