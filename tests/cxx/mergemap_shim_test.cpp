// mergemap_shim_test.cpp -- include/shim/app/CoSLAMMergeConstraints.h through mergeMapPoints: the scene is loaded as
// tests/cxx/mergeconstraints_shim_test.cpp loads it, genMergeInfoVer2 runs (assembly, the two solves, the MergeInfo list) and the merge list
// and the solved points are applied to the live tables.  tests/test_mergemap_shim_gpu.py compiles it with g++, writes <in.bin>
// (tests/mergeconstraints_scenes.py write_input: one scene behind an int 1) and compares <out.bin> with coslam_amd.MergeCamGroups on the same
// data (the same kernels and solves: bit for bit).  pointFeat is derived here as the reference's slot where its frame is the current one,
// refStatic is the pattern (37 m + 11 c + 1) % 251 of tests/mergemap_dev.py.
//   mergemap_shim_test <in.bin> <out.bin>
// out: int ok, verdict, nInfo, nMap, nCams, N; int counts[6]; slot2map [nCams][N]; featRef [nMap][nCams][4]; pointFeat [nMap][nCams];
//      refStatic [nMap][nCams] (bytes); M [nMap][3] (doubles)
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "app/CoSLAMMergeConstraints.h"

#define HIPOK(x)                                          \
    do {                                                  \
        if ((x) != hipSuccess) {                          \
            fprintf(stderr, "HIP call failed: %s\n", #x); \
            return 3;                                     \
        }                                                 \
    } while (0)

template <class T> static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
template <class T> static T* up(const std::vector<T>& v) {
    T* d = 0;
    if (hipMalloc((void**)&d, v.size() * sizeof(T) + 8) != hipSuccess) return 0;
    if (!v.empty() && hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return 0;
    return d;
}
struct Match {
    int idx1, idx2;
};
struct Matching {   // the members of the reference's Matching that genMergeInfoVer2 reads
    int num;
    std::vector<Match> data;
    const Match& operator[](int i) const { return data[i]; }
};

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int one = 0, h12[12];
    if (!f || !rd(f, &one, 1) || one != 1 || !rd(f, h12, 12)) return 2;
    const int nCams = h12[0], N = h12[1], nMap = h12[2], nF = h12[3], frame0 = h12[4], nKey = h12[5], nGroup = h12[6], gId1 = h12[7], gId2 = h12[8],
              iCam = h12[9], jCam = h12[10], nMatch = h12[11];
    std::vector<int> frames(nKey), selfI((size_t)nKey * nCams);
    if (!rd(f, frames.data(), nKey) || !rd(f, selfI.data(), selfI.size())) return 2;
    std::vector<unsigned char> self(selfI.begin(), selfI.end());
    cs_camera_groups G;
    memset(&G, 0xFF, sizeof(G));
    G.groupNum = nGroup;
    for (int g = 0; g < 16; ++g) G.num[g] = 0;
    for (int g = 0; g < nGroup; ++g) {
        if (!rd(f, &G.num[g], 1) || !rd(f, G.camIds[g], G.num[g])) return 2;
        for (int i = 0; i < G.num[g]; ++i) G.groupId[G.camIds[g][i]] = g;
    }
    std::vector<double> K(9 * nCams), RT((size_t)nCams * nF * 12), M(3 * (size_t)nMap), xy((size_t)nCams * nF * 2 * N);
    std::vector<int> state((size_t)nCams * N), s2m((size_t)nCams * N), ref((size_t)nMap * nCams * 4), matches(2 * (size_t)nMatch);
    if (!rd(f, K.data(), K.size()) || !rd(f, RT.data(), RT.size()) || !rd(f, M.data(), M.size()) || !rd(f, state.data(), state.size()) ||
        !rd(f, s2m.data(), s2m.size()) || !rd(f, xy.data(), xy.size()) || !rd(f, ref.data(), ref.size()))
        return 2;
    std::vector<std::vector<int> > segs(nCams);
    int nSeg = 0;
    for (int c = 0; c < nCams; ++c) {
        int n;
        if (!rd(f, &n, 1)) return 2;
        segs[c].resize(4 * (size_t)n);
        if (!rd(f, segs[c].data(), segs[c].size())) return 2;
        nSeg = n > nSeg ? n : nSeg;
    }
    if (!rd(f, matches.data(), matches.size())) return 2;
    fclose(f);

    // the history: every frame pushed with its pixels and poses (cs_detect_dynamic_dev pushes; minLen switches its test off), the segments
    cs_track_history* h = cs_track_history_create_ex(0, nCams, N, 16, nF > 16 ? nF : 16);
    if (!h) return 1;
    std::vector<double> KiK(18 * (size_t)nCams);
    for (int c = 0; c < nCams; ++c) {
        const double* k = &K[9 * c];
        const double iK[9] = {1 / k[0], -k[1] / (k[0] * k[4]), (k[1] * k[5] - k[2] * k[4]) / (k[0] * k[4]), 0, 1 / k[4], -k[5] / k[4], 0, 0, 1};
        memcpy(&KiK[18 * c], k, 72), memcpy(&KiK[18 * c + 9], iK, 72);
    }
    double *dK = up(KiK), *dXY = up(xy), *dM = up(M);
    int *dState = up(state), *dS2m = up(s2m), *dRef = up(ref);
    std::vector<int> none((size_t)N, -1), span(2 * (size_t)N, -1), tracked((size_t)nCams * nF * N);
    for (size_t c = 0; c < (size_t)nCams * nF; ++c)
        for (int s = 0; s < N; ++s) tracked[c * N + s] = xy[c * 2 * N + s] != -1.0 ? 0 : -1;
    int *dNone = up(none), *dSpan = up(span), *dTracked = up(tracked);
    std::vector<unsigned char> ones((size_t)N, 1), zero1(1, 0);
    unsigned char *dStat = up(ones), *dFl = up(zero1);
    cs_camera_groups* dG = 0;
    HIPOK(hipMalloc((void**)&dG, sizeof(G))); HIPOK(hipMemcpy(dG, &G, sizeof(G), hipMemcpyHostToDevice));
    double *dR, *dT;
    HIPOK(hipMalloc((void**)&dR, nCams * 72)); HIPOK(hipMalloc((void**)&dT, nCams * 24));
    if (!dK || !dXY || !dM || !dState || !dS2m || !dRef || !dNone || !dSpan || !dTracked || !dStat || !dFl) return 3;
    std::vector<cs_poseupdate_cam> pc(nCams);
    std::vector<double> fR(nCams * 9), fT(nCams * 3);
    for (int i = 0; i < nF; ++i) {
        for (int c = 0; c < nCams; ++c) {
            const size_t ci = (size_t)c * nF + i;
            cs_poseupdate_cam q = {dK + 18 * c, dK + 18 * c + 9, dXY + ci * 2 * N, dTracked + ci * N, dNone, dSpan, 0, dStat};
            pc[c] = q;
            memcpy(&fR[9 * c], &RT[ci * 12], 72), memcpy(&fT[3 * c], &RT[ci * 12 + 9], 24);
        }
        HIPOK(hipMemcpy(dR, fR.data(), fR.size() * 8, hipMemcpyHostToDevice)); HIPOK(hipMemcpy(dT, fT.data(), fT.size() * 8, hipMemcpyHostToDevice));
        if (cs_detect_dynamic_dev(h, 0, 0, nCams, pc.data(), dR, dT, 1, dFl, frame0 + i, 20, 1 << 30, 3, 6.0, 0) != CS_OK) {
            fprintf(stderr, "%s\n", cs_last_error());
            return 1;
        }
        HIPOK(hipDeviceSynchronize());
    }
    if (nSeg > 0) {
        std::vector<cs_feat_seg> pool((size_t)nCams * nSeg);
        memset(pool.data(), 0xFF, pool.size() * sizeof(cs_feat_seg));
        for (int c = 0; c < nCams; ++c) memcpy(&pool[(size_t)c * nSeg], segs[c].data(), segs[c].size() * 4);
        if (cs_track_history_load_segments(h, pool.data(), nSeg) != CS_OK) return 1;
    }

    int rc = 0;
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    try {
        CoSLAMMergeConstraints merger(nCams, N, nMatch > 0 ? nMatch : 1, nMap, h);
        for (int c = 0; c < nCams; ++c) {
            cs_merge_cam cam = {dXY + ((size_t)c * nF + nF - 1) * 2 * N, dState + (size_t)c * N, dS2m + (size_t)c * N, dK + 18 * c, 0, 0};
            merger.setCamera(c, cam);
            merger.storeFeaturePoints(c, &state[(size_t)c * N]);
        }
        merger.setMap((const cs_feat_ref*)dRef, dM);
        merger.setKeyFrames(nKey, frames.data(), self.data());
        merger.setCurrentFrame(G, dG);
        // slot pairs -> the reference's list indices (the rank of a slot among the features of its camera)
        std::vector<int> rank((size_t)nCams * N, -1);
        for (int c = 0; c < nCams; ++c)
            for (int s = 0, r = 0; s < N; ++s)
                if (state[(size_t)c * N + s] == 0 || state[(size_t)c * N + s] == 1) rank[(size_t)c * N + s] = r++;
        Matching fm;
        for (int k = 0; k < nMatch; ++k) {
            const Match m = {rank[(size_t)iCam * N + matches[2 * k]], rank[(size_t)jCam * N + matches[2 * k + 1]]};
            fm.data.push_back(m);
        }
        fm.num = (int)fm.data.size();
        const bool ok = merger.genMergeInfoVer2(gId1, gId2, iCam, jCam, fm);
        const cs_merge_constraints_header& H = merger.header;
        const int f2 = frame0 + nF - 1;
        std::vector<int> pf((size_t)nMap * nCams), cnt(6, 0);
        std::vector<unsigned char> rs((size_t)nMap * nCams);
        for (int m = 0; m < nMap; ++m)
            for (int c = 0; c < nCams; ++c) {
                const int* r = &ref[((size_t)m * nCams + c) * 4];
                pf[(size_t)m * nCams + c] = r[0] >= 0 && r[1] == f2 ? r[0] : -1;
                rs[(size_t)m * nCams + c] = (unsigned char)((37 * m + 11 * c + 1) % 251);
            }
        int *dPf = up(pf), *dCnt = up(cnt);
        unsigned char* dRs = up(rs);
        if (!dPf || !dCnt || !dRs) return 3;
        merger.mergeMapPoints(dPf, (cs_feat_ref*)dRef, dRs, dM, true, dCnt);   // behind a rejected verdict too: it must change nothing
        HIPOK(hipDeviceSynchronize());
        HIPOK(hipMemcpy(cnt.data(), dCnt, 24, hipMemcpyDeviceToHost));
        HIPOK(hipMemcpy(s2m.data(), dS2m, s2m.size() * 4, hipMemcpyDeviceToHost));
        HIPOK(hipMemcpy(ref.data(), dRef, ref.size() * 4, hipMemcpyDeviceToHost));
        HIPOK(hipMemcpy(pf.data(), dPf, pf.size() * 4, hipMemcpyDeviceToHost));
        HIPOK(hipMemcpy(rs.data(), dRs, rs.size(), hipMemcpyDeviceToHost));
        HIPOK(hipMemcpy(M.data(), dM, M.size() * 8, hipMemcpyDeviceToHost));
        const int head[6] = {ok ? 1 : 0, H.verdict, merger.m_nMergeInfo, nMap, nCams, N};
        fwrite(head, 4, 6, o), fwrite(cnt.data(), 4, 6, o), fwrite(s2m.data(), 4, s2m.size(), o), fwrite(ref.data(), 4, ref.size(), o);
        fwrite(pf.data(), 4, pf.size(), o), fwrite(rs.data(), 1, rs.size(), o), fwrite(M.data(), 8, M.size(), o);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        rc = 1;
    }
    fclose(o);
    cs_track_history_destroy(h);
    return rc;
}
