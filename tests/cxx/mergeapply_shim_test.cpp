// mergeapply_shim_test.cpp -- include/shim/app/CoSLAMMergeApply.h driven the way CoSLAM::mergeCamGroups would (reference
// src/app/SL_CoSLAM.cpp:1405-1437): a history is filled through the C-ABI, the shim plans, corrects the poses, merges the groups and
// re-triangulates; the span of the history and the groups go to <out.bin>.  tests/test_mergeapply_gpu.py compiles it with g++, writes
// <in.bin> and compares <out.bin> with MergeApply's result on the same data (the same kernels: bit for bit):
//   mergeapply_shim_test <in.bin> <out.bin>
// in:  int nCams, nFrames, frame0, nKey, firstConstrain, camid1, camid2, nInfo; int frames[nKey]; per key frame a cs_camera_groups; per info
//      int frame1, cam1, frame2, cam2, gid1, gid2; double infoR[nInfo][9], infoT[nInfo][3]; double R[nCams][nFrames][9], t[nCams][nFrames][3]
// out: double R[nCams][nFrames][9], t[nCams][nFrames][3]; cs_camera_groups (merged); int groupId[16], mergedGid, firstFrame, lastFrame
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "app/CoSLAMMergeApply.h"

#define HIPOK(x)                                                 \
    do {                                                         \
        if ((x) != hipSuccess) {                                 \
            fprintf(stderr, "HIP call failed: %s\n", #x);        \
            return 3;                                            \
        }                                                        \
    } while (0)

template <class T> static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int h8[8];
    if (!rd(f, h8, 8)) return 2;
    const int nCams = h8[0], nFrames = h8[1], frame0 = h8[2], nKey = h8[3], firstConstrain = h8[4], camid1 = h8[5], camid2 = h8[6], nInfo = h8[7];
    std::vector<int> frames(nKey), infos(4 * nInfo), gid1(nInfo), gid2(nInfo);
    std::vector<cs_camera_groups> groups(nKey);
    if (!rd(f, frames.data(), nKey) || !rd(f, groups.data(), nKey)) return 2;
    for (int i = 0; i < nInfo; ++i) {
        int v[6];
        if (!rd(f, v, 6)) return 2;
        memcpy(&infos[4 * i], v, 16), gid1[i] = v[4], gid2[i] = v[5];
    }
    std::vector<double> infoR(9 * nInfo), infoT(3 * nInfo), R((size_t)nCams * nFrames * 9), T((size_t)nCams * nFrames * 3);
    if (!rd(f, infoR.data(), infoR.size()) || !rd(f, infoT.data(), infoT.size()) || !rd(f, R.data(), R.size()) || !rd(f, T.data(), T.size())) return 2;
    fclose(f);

    // a history of one slot per camera: every frame pushed (cs_detect_dynamic_dev pushes; minLen switches its test off), then the poses
    const int N = 1;
    cs_track_history* h = cs_track_history_create_ex(0, nCams, N, 16, nFrames > 16 ? nFrames : 16);
    if (!h) {
        fprintf(stderr, "%s\n", cs_last_error());
        return 1;
    }
    double *dK, *dXY, *dR, *dT, *dPoseR, *dPoseT, *dInfoR, *dInfoT, *dM, *dCov;
    int *dState, *dS2m, *dSpan, *dFrames, *dCnt;
    unsigned char *dStat, *dFl;
    cs_feat_ref* dRef;
    const double K[9] = {520, 0, 320, 0, 515, 240, 0, 0, 1}, iK[9] = {1 / 520.0, 0, -320 / 520.0, 0, 1 / 515.0, -240 / 515.0, 0, 0, 1};
    HIPOK(hipMalloc((void**)&dK, 18 * 8)); HIPOK(hipMemcpy(dK, K, 72, hipMemcpyHostToDevice)); HIPOK(hipMemcpy(dK + 9, iK, 72, hipMemcpyHostToDevice));
    HIPOK(hipMalloc((void**)&dXY, 16)); HIPOK(hipMemset(dXY, 0, 16));
    HIPOK(hipMalloc((void**)&dState, 4)); HIPOK(hipMemset(dState, 0xFF, 4));
    HIPOK(hipMalloc((void**)&dS2m, 4)); HIPOK(hipMemset(dS2m, 0xFF, 4));
    HIPOK(hipMalloc((void**)&dSpan, 8)); HIPOK(hipMemset(dSpan, 0xFF, 8));
    HIPOK(hipMalloc((void**)&dStat, 1)); HIPOK(hipMemset(dStat, 1, 1));
    HIPOK(hipMalloc((void**)&dFl, 1)); HIPOK(hipMemset(dFl, 0, 1));
    HIPOK(hipMalloc((void**)&dR, nCams * 72)); HIPOK(hipMalloc((void**)&dT, nCams * 24));
    std::vector<cs_poseupdate_cam> cams(nCams);
    for (int c = 0; c < nCams; ++c) {
        cs_poseupdate_cam q = {dK, dK + 9, dXY, dState, dS2m, dSpan, 0, dStat};
        cams[c] = q;
    }
    std::vector<double> fR(nCams * 9), fT(nCams * 3);
    for (int i = 0; i < nFrames; ++i) {
        for (int c = 0; c < nCams; ++c) {
            memcpy(&fR[9 * c], &R[((size_t)c * nFrames + i) * 9], 72);
            memcpy(&fT[3 * c], &T[((size_t)c * nFrames + i) * 3], 24);
        }
        HIPOK(hipMemcpy(dR, fR.data(), fR.size() * 8, hipMemcpyHostToDevice)); HIPOK(hipMemcpy(dT, fT.data(), fT.size() * 8, hipMemcpyHostToDevice));
        if (cs_detect_dynamic_dev(h, 0, 0, nCams, cams.data(), dR, dT, 1, dFl, frame0 + i, 20, 1 << 30, 3, 6.0, 0) != CS_OK) {
            fprintf(stderr, "%s\n", cs_last_error());
            return 1;
        }
        HIPOK(hipDeviceSynchronize());
    }
    HIPOK(hipMalloc((void**)&dInfoR, infoR.size() * 8 + 8)); HIPOK(hipMalloc((void**)&dInfoT, infoT.size() * 8 + 8));
    HIPOK(hipMemcpy(dInfoR, infoR.data(), infoR.size() * 8, hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(dInfoT, infoT.data(), infoT.size() * 8, hipMemcpyHostToDevice));
    // one map row without features: the re-triangulation runs, selects it and leaves it alone
    std::vector<cs_feat_ref> ref(nCams);
    for (int c = 0; c < nCams; ++c) ref[c].slot = -1, ref[c].frame = 0, ref[c].first = 0, ref[c].seg = -1;
    HIPOK(hipMalloc((void**)&dRef, nCams * sizeof(cs_feat_ref))); HIPOK(hipMemcpy(dRef, ref.data(), nCams * sizeof(cs_feat_ref), hipMemcpyHostToDevice));
    HIPOK(hipMalloc((void**)&dM, 24)); HIPOK(hipMemset(dM, 0, 24)); HIPOK(hipMalloc((void**)&dCov, 72)); HIPOK(hipMemset(dCov, 0, 72));
    HIPOK(hipMalloc((void**)&dFrames, 8)); HIPOK(hipMalloc((void**)&dCnt, 16)); HIPOK(hipMemset(dCnt, 0, 16));
    const int ff[2] = {frame0, frame0 + nFrames - 1};
    HIPOK(hipMemcpy(dFrames, ff, 8, hipMemcpyHostToDevice));

    cs_camera_groups cur = groups.back();
    int groupId[16], mergedGid = -1, cnt[4] = {0, 0, 0, 0};
    HIPOK(hipMalloc((void**)&dPoseR, R.size() * 8)); HIPOK(hipMalloc((void**)&dPoseT, T.size() * 8));
    try {
        CoSLAMMergeApply mcg(nCams, h);
        mcg.setKeyFrames(nKey, frames.data(), groups.data(), firstConstrain);
        mcg.setMergeInfo(nInfo, infos.data(), gid1.data(), gid2.data(), dInfoR, dInfoT, camid1, camid2);
        mcg.searchFirstKeyFrameForMerge();
        mcg.recomputeKeyCamPoses();
        mcg.recomputeAllCameraPoses();
        mergedGid = mcg.mergeMatchedGroups(&cur, groupId);
        mcg.recomputeMapPoints(cams.data(), dRef, 1, 0, dFrames, dFrames + 1, dFl, mcg.getFirstFrame(), dM, dCov, 3.0, dCnt);
        mcg.wait();
        HIPOK(hipMemcpy(cnt, dCnt, 16, hipMemcpyDeviceToHost));
        if (cnt[0] != 1 || cnt[1] != 0 || cnt[2] != 1) {
            fprintf(stderr, "recomputeMapPoints counted %d %d %d %d\n", cnt[0], cnt[1], cnt[2], cnt[3]);
            return 1;
        }
        if (cs_track_history_get_span_dev(h, 0, frame0, nFrames, dPoseR, dPoseT) != CS_OK) throw std::runtime_error(cs_last_error());
        HIPOK(hipDeviceSynchronize());
        HIPOK(hipMemcpy(R.data(), dPoseR, R.size() * 8, hipMemcpyDeviceToHost)); HIPOK(hipMemcpy(T.data(), dPoseT, T.size() * 8, hipMemcpyDeviceToHost));
        const int tail[4] = {mergedGid, mcg.getFirstFrame(), mcg.getLastFrame(), 0};
        FILE* o = fopen(argv[2], "wb");
        if (!o) return 2;
        fwrite(R.data(), 8, R.size(), o), fwrite(T.data(), 8, T.size(), o), fwrite(&cur, sizeof(cur), 1, o), fwrite(groupId, 4, 16, o);
        fwrite(tail, 4, 3, o);
        fclose(o);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    cs_track_history_destroy(h);
    return 0;
}
