// ref_mergeconstraints_test.cpp -- the reference's OWN MergeCameraGroup::genMergeInfoVer2 (src/app/SL_MergeCameraGroup.cpp:557-725) with
// its helpers getCamIdsInBothGroups, buildIdMapForSelfKeyPoses, getCorresFeatPtsAndMapPts, checkMergeMapPoints, mergeMapPoints,
// getUnMergedFeatureTracks, getCorresFeatPtsInPrevSelfKeyPoses and getRigidTransFromToWithEMat, on KeyFrame / KeyPose / FeaturePoint /
// MapPoint objects built from scene files: the fixture that pins cs_merge_first_constrain and cs_merge_constraints_assemble_dev
// (DESIGN 3.22).
//
// bundleAdjustRobust has no source in the reference tree, so the pin stops at the solver call and starts again behind it: this driver
// defines the function itself (the declaration of tests/cxx/ref_shim_merge/ref_merge_offpath.h), records the arguments of the first call and
// changes nothing.  The MergeInfo list that follows is therefore the relative poses of the UNSOLVED poses.
//
// A scene is given in the library's own terms (tests/golden/make_mergeconstraints_golden.py): per camera the current key frame's slot
// tables (state, slot2map), the history's pixels and poses for frame0 .. f2, the references featRef [nMap][nCams] with the cameras' linked
// segments, the map, the key frames with their self-motion flags, the groups of the current key frame and the matches as SLOT pairs.  The
// driver turns them into the reference's objects: m_featPoints[c] = the slots with state 0 / 1 in slot order (a match's list index is the
// slot's rank); MapPoint::pFeatures[c] = the head of featRef[m][c] with its preFrame chain (the run [first, frame] on the slot, then the
// segments); a tracked slot whose slot2map names the point of such a head AT f2 is that head.  MapPoint::numVisCam is brought up to date
// with updateVisCamNum(f2) when the scene is built -- the frame loop keeps it so, and getUnMergedFeatureTracks reads it as stored.
// Un-vendored on the path and OUR definitions: sortWithInd (stable, descending), matEyes, matZeros, and -- already in oracle/ref_shim --
// project, dist2 (the Euclidean distance of two pixels), getRigidTransFromTo, formEMat.
//   ref_mergeconstraints_test golden <in.bin> <out.bin>          CPU only
// Built by oracle/Makefile, target _ref/ref_mergeconstraints_test (where the reference tree exists; the Makefile's header lists the
// three expressions of SL_MergeCameraGroup.cpp that are rewritten in the compile pipe).
// TEST INFRASTRUCTURE; the binary goes to oracle/_ref/ (untracked), nothing on the GPU side needs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <vector>

#include "app/SL_MergeCameraGroup.h"
#include "slam/SL_KeyPoseList.h"

// ---- un-vendored helpers on the path: our definitions ----
void sortWithInd(int n, int* vals, int* ind, bool ascending) {   // stable
    std::vector<std::pair<int, int> > v(n);
    for (int i = 0; i < n; ++i) v[i] = std::make_pair(vals[i], ind[i]);
    if (ascending)
        std::stable_sort(v.begin(), v.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) { return a.first < b.first; });
    else
        std::stable_sort(v.begin(), v.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) { return a.first > b.first; });
    for (int i = 0; i < n; ++i) vals[i] = v[i].first, ind[i] = v[i].second;
}
void matEyes(int n, Mat_d& I) {
    I.resize(n, n);
    I.fill(0);
    for (int i = 0; i < n; ++i) I.data[i * n + i] = 1;
}
void matZeros(int m, int n, Mat_d& Z) {
    Z.resize(m, n);
    Z.fill(0);
}

// ---- the solver stand-in ----
struct Recorded {
    int calls, nCamsCon[2], nPtsCon[2], maxIter[2], inner[2];
    double maxErr[2];
    std::vector<double> K, R, T, pts, xy;
    std::vector<int> ptr, cam;
};
static Recorded g_rec;
void bundleAdjustRobust(int nCamsCon, std::vector<Mat_d>& Ks, std::vector<Mat_d>& Rs, std::vector<Mat_d>& Ts, int nPtsCon,
                        std::vector<Point3d>& pts, std::vector<std::vector<Meas2D> >& meas, double maxErr, int maxIter, int innerMaxIter) {
    const int k = g_rec.calls++;
    if (k < 2) g_rec.nCamsCon[k] = nCamsCon, g_rec.nPtsCon[k] = nPtsCon, g_rec.maxIter[k] = maxIter, g_rec.inner[k] = innerMaxIter, g_rec.maxErr[k] = maxErr;
    if (k) return;
    for (size_t j = 0; j < Rs.size(); ++j) {
        g_rec.K.insert(g_rec.K.end(), Ks[j].data, Ks[j].data + 9);
        g_rec.R.insert(g_rec.R.end(), Rs[j].data, Rs[j].data + 9);
        g_rec.T.insert(g_rec.T.end(), Ts[j].data, Ts[j].data + 3);
    }
    g_rec.ptr.push_back(0);
    for (size_t i = 0; i < pts.size(); ++i) {
        g_rec.pts.insert(g_rec.pts.end(), pts[i].M, pts[i].M + 3);
        for (size_t m = 0; m < meas[i].size(); ++m) g_rec.cam.push_back(meas[i][m].viewId), g_rec.xy.push_back(meas[i][m].x), g_rec.xy.push_back(meas[i][m].y);
        g_rec.ptr.push_back((int)g_rec.cam.size());
    }
}

template <class T> static void get(FILE* f, T* p, size_t n) {
    if (fread(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "ref_mergeconstraints_test: short input\n");
        exit(1);
    }
}
static int geti(FILE* f) {
    int v;
    get(f, &v, 1);
    return v;
}
template <class T> static void put(FILE* f, const T* p, size_t n) { fwrite(p, sizeof(T), n, f); }
static void puti(FILE* f, int v) { fwrite(&v, 4, 1, f); }
static void fail(const char* what, int sc) {
    fprintf(stderr, "ref_mergeconstraints_test: scene %d: %s\n", sc, what);
    exit(1);
}

struct Node {
    int cam, frame, slot;
};

int main(int argc, char** argv) {
    if (argc < 4 || strcmp(argv[1], "golden")) {
        fprintf(stderr, "usage: %s golden <in.bin> <out.bin>\n", argv[0]);
        return 2;
    }
    FILE* in = fopen(argv[2], "rb");
    FILE* out = fopen(argv[3], "wb");
    if (!in || !out) return 1;
    const int nScenes = geti(in);
    for (int sc = 0; sc < nScenes; ++sc) {
        const int nCams = geti(in), N = geti(in), nMap = geti(in), nFrames = geti(in), frame0 = geti(in), nKey = geti(in), nGroup = geti(in),
                  gId1 = geti(in), gId2 = geti(in), maxiCam = geti(in), maxjCam = geti(in), nMatch = geti(in);
        if (nCams < 1 || nCams > SLAM_MAX_NUM) fail("the reference holds at most SLAM_MAX_NUM cameras", sc);
        const int f2 = frame0 + nFrames - 1;
        std::vector<int> keyFrames(nKey), selfMotion((size_t)nKey * nCams);
        get(in, keyFrames.data(), nKey), get(in, selfMotion.data(), selfMotion.size());
        if (keyFrames[nKey - 1] != f2 || keyFrames[0] < frame0) fail("the key frames must lie in the store and end at its newest frame", sc);
        CameraGroup groups[SLAM_MAX_NUM];
        for (int g = 0; g < nGroup; ++g) {
            const int n = geti(in);
            for (int i = 0; i < n; ++i) groups[g].addCam(geti(in));
        }
        std::vector<double> K(9 * nCams), R((size_t)9 * nCams * nFrames), T((size_t)3 * nCams * nFrames), M(3 * (size_t)nMap);
        get(in, K.data(), K.size());
        for (int c = 0; c < nCams; ++c)
            for (int i = 0; i < nFrames; ++i) get(in, &R[9 * ((size_t)c * nFrames + i)], 9), get(in, &T[3 * ((size_t)c * nFrames + i)], 3);
        get(in, M.data(), M.size());
        std::vector<int> state((size_t)nCams * N), slot2map((size_t)nCams * N), featRef((size_t)nMap * nCams * 4);
        std::vector<double> xy((size_t)nCams * nFrames * 2 * N);
        get(in, state.data(), state.size()), get(in, slot2map.data(), slot2map.size()), get(in, xy.data(), xy.size());
        get(in, featRef.data(), featRef.size());
        std::vector<std::vector<int> > segs(nCams);
        for (int c = 0; c < nCams; ++c) {
            const int n = geti(in);
            segs[c].resize(4 * (size_t)n);
            get(in, segs[c].data(), segs[c].size());
        }
        std::vector<int> matches(2 * (size_t)nMatch);
        get(in, matches.data(), matches.size());

        // ---- the reference's objects ----
        std::vector<std::vector<CamPoseItem*> > poses(nCams, std::vector<CamPoseItem*>(nFrames));
        for (int c = 0; c < nCams; ++c)
            for (int i = 0; i < nFrames; ++i) {
                CamPoseItem* p = poses[c][i] = new CamPoseItem();
                p->f = frame0 + i, p->camId = c;
                memcpy(p->R, &R[9 * ((size_t)c * nFrames + i)], 72), memcpy(p->t, &T[3 * ((size_t)c * nFrames + i)], 24);
            }
        std::vector<KeyFrame*> kfs(nKey);
        for (int k = 0; k < nKey; ++k) {
            KeyFrame* kf = kfs[k] = new KeyFrame(keyFrames[k]);
            kf->setCamNum(nCams);
            kf->setCamGroups(groups, nGroup);
            for (int c = 0; c < nCams; ++c) {
                KeyPose* kp = new KeyPose(keyFrames[k], poses[c][keyFrames[k] - frame0]);
                kp->setCameraIntrinsic(&K[9 * c]);
                kp->bSelfMotion = selfMotion[(size_t)k * nCams + c] != 0;
                kf->setKeyPose(c, kp);
            }
            if (k) kf->prev = kfs[k - 1], kfs[k - 1]->next = kf;
        }
        std::map<FeaturePoint*, Node> nodeOf;
        std::vector<FeaturePoint*> all;
        auto newFeat = [&](int c, int fr, int slot, MapPoint* mp) {
            const bool held = fr >= frame0 && fr <= f2;
            const double* row = held ? &xy[((size_t)c * nFrames + (fr - frame0)) * 2 * N] : 0;
            FeaturePoint* fp = new FeaturePoint(fr, c, held ? row[slot] : 0.0, held ? row[N + slot] : 0.0);
            fp->setIntrinsic(&K[9 * c]);
            if (held) fp->setCameraPose(poses[c][fr - frame0]);
            fp->mpt = mp, fp->preFrame = fp->nextFrame = 0;
            const Node nd = {c, fr, slot};
            nodeOf[fp] = nd;
            all.push_back(fp);
            return fp;
        };
        std::vector<MapPoint*> pts(nMap);
        std::map<MapPoint*, int> indexOf;
        std::vector<std::vector<FeaturePoint*> > cur(nCams, std::vector<FeaturePoint*>(N, (FeaturePoint*)0));
        for (int m = 0; m < nMap; ++m) {
            MapPoint* mp = pts[m] = new MapPoint(M[3 * m], M[3 * m + 1], M[3 * m + 2], f2);
            mp->setLocalStatic();
            indexOf[mp] = m;
            for (int c = 0; c < nCams; ++c) {
                const int* r = &featRef[((size_t)m * nCams + c) * 4];
                if (r[0] < 0) continue;
                FeaturePoint* newer = 0;
                int slot = r[0], last = r[1], first = r[2], seg = r[3], hops = 0;
                for (;;) {
                    for (int fr = last; fr >= first; --fr) {
                        FeaturePoint* fp = newFeat(c, fr, slot, mp);
                        if (newer) newer->preFrame = fp, fp->nextFrame = newer;
                        else mp->pFeatures[c] = fp;
                        newer = fp;
                    }
                    if (seg < 0 || 4 * (size_t)seg >= segs[c].size() || ++hops > 100000) break;
                    const int* s = &segs[c][4 * (size_t)seg];
                    slot = s[0], last = s[1], first = s[2], seg = s[3];
                }
                if (r[1] == f2) {
                    if (r[0] >= N || (state[(size_t)c * N + r[0]] != 0 && state[(size_t)c * N + r[0]] != 1) || slot2map[(size_t)c * N + r[0]] != m)
                        fail("a reference at the current frame must be a tracked slot of its point", sc);
                    cur[c][r[0]] = mp->pFeatures[c];
                }
            }
            mp->updateVisCamNum(f2);
        }
        MergeCameraGroup* mcg = new MergeCameraGroup();
        mcg->setCurrentFrame(kfs[nKey - 1]);
        std::vector<std::vector<int> > rank(nCams, std::vector<int>(N, -1));
        for (int c = 0; c < nCams; ++c)
            for (int s = 0; s < N; ++s) {
                const int st = state[(size_t)c * N + s];
                if (st != 0 && st != 1) continue;
                if (!cur[c][s]) {
                    if (slot2map[(size_t)c * N + s] >= 0) fail("a mapped slot must be its point's reference at the current frame", sc);
                    cur[c][s] = newFeat(c, f2, s, 0);
                }
                rank[c][s] = (int)mcg->m_featPoints[c].size();
                mcg->m_featPoints[c].push_back(cur[c][s]);
            }
        Matching featMatches;
        for (int i = 0; i < nMatch; ++i) {
            const int a = matches[2 * i], b = matches[2 * i + 1];
            if (a < 0 || a >= N || b < 0 || b >= N || rank[maxiCam][a] < 0 || rank[maxjCam][b] < 0) fail("a match names a slot that is no feature", sc);
            featMatches.add(rank[maxiCam][a], rank[maxjCam][b], 0.0);
        }
        std::vector<MapPoint*> before(all.size());
        for (size_t i = 0; i < all.size(); ++i) before[i] = all[i]->mpt;

        // ---- the call; avg_err is only printed (:460), so it is read back from the stream at full precision ----
        g_rec = Recorded();
        std::ostringstream log;
        std::streambuf* old = std::cout.rdbuf(log.rdbuf());
        std::cout.precision(17);
        const bool ok = mcg->genMergeInfoVer2(gId1, gId2, maxiCam, maxjCam, featMatches);
        std::cout.rdbuf(old);
        const std::string text = log.str();
        const size_t at = text.find("avg_err:");
        if (at == std::string::npos) fail("no avg_err in the log", sc);
        const double avgErr = strtod(text.c_str() + at + 8, 0);

        puti(out, ok ? 1 : 0);
        put(out, &avgErr, 1);
        puti(out, mcg->m_pFirstConstrainFrm->f);
        const int nPose = (int)mcg->order_to_pose.size();
        puti(out, nPose);
        for (int n = 0; n < nPose; ++n) puti(out, mcg->order_to_pose[n]->cam->f), puti(out, mcg->order_to_pose[n]->cam->camId);
        puti(out, g_rec.calls);
        if (g_rec.calls) {
            for (int k = 0; k < 2; ++k)
                puti(out, g_rec.nCamsCon[k]), puti(out, g_rec.nPtsCon[k]), puti(out, g_rec.maxIter[k]), puti(out, g_rec.inner[k]), put(out, &g_rec.maxErr[k], 1);
            const int C = (int)g_rec.T.size() / 3, P = (int)g_rec.pts.size() / 3, nObs = (int)g_rec.cam.size();
            puti(out, C), puti(out, P), puti(out, nObs);
            put(out, g_rec.K.data(), g_rec.K.size()), put(out, g_rec.R.data(), g_rec.R.size()), put(out, g_rec.T.data(), g_rec.T.size());
            put(out, g_rec.pts.data(), g_rec.pts.size());
            for (int i = 0; i < P; ++i) {   // which map point: the coordinates are unique in a scene
                int hit = -1, nHit = 0;
                for (int m = 0; m < nMap; ++m)
                    if (!memcmp(&g_rec.pts[3 * i], &M[3 * m], 24)) hit = m, ++nHit;
                if (nHit != 1) fail("a recorded point is not exactly one map point", sc);
                puti(out, hit);
            }
            put(out, g_rec.ptr.data(), g_rec.ptr.size()), put(out, g_rec.cam.data(), g_rec.cam.size()), put(out, g_rec.xy.data(), g_rec.xy.size());
        }
        puti(out, mcg->m_nMergeInfo);
        for (int i = 0; i < mcg->m_nMergeInfo; ++i) {
            const MergeInfo& mi = mcg->m_mergeInfo[i];
            const int v[7] = {mi.frame1, mi.camId1, mi.groupId1, mi.frame2, mi.camId2, mi.groupId2, mi.valid ? 1 : 0};
            put(out, v, 7), put(out, mi.E, 9), put(out, mi.R, 9), put(out, mi.t, 3);
        }
        // ---- the post-state ----
        for (int c = 0; c < nCams; ++c)
            for (int s = 0; s < N; ++s) puti(out, cur[c][s] && cur[c][s]->mpt ? indexOf[cur[c][s]->mpt] : -1);
        for (int m = 0; m < nMap; ++m)
            for (int c = 0; c < nCams; ++c) {
                FeaturePoint* fp = pts[m]->pFeatures[c];
                puti(out, fp ? nodeOf[fp].slot : -1), puti(out, fp ? nodeOf[fp].frame : -1);
            }
        std::vector<int> det;
        for (size_t i = 0; i < all.size(); ++i)
            if (before[i] && !all[i]->mpt) {
                const Node& nd = nodeOf[all[i]];
                det.push_back(nd.cam), det.push_back(nd.frame), det.push_back(nd.slot);
            }
        puti(out, (int)det.size() / 3);
        put(out, det.data(), det.size());
        printf("  scene %d: %d cameras, %d matches -> %s, avg_err %.6g, first-constrained frame %d, %d poses, %d points, %d measurements, %d infos, %d detached\n",
               sc, nCams, nMatch, ok ? "merge" : "REJECT", avgErr, mcg->m_pFirstConstrainFrm->f, nPose, (int)g_rec.pts.size() / 3, (int)g_rec.cam.size(),
               mcg->m_nMergeInfo, (int)det.size() / 3);
    }
    fclose(in), fclose(out);
    printf("ref_mergeconstraints_test: %d scenes\n", nScenes);
    return 0;
}
