// ref_mergeapply_test.cpp -- the reference's OWN CoSLAM::getMapPts (src/app/SL_CoSLAM.cpp:1818-1851) and
// updateStaticPointPositionAtKeyFrms (src/slam/SL_CoSLAMHelper.cpp:395-451; what MergeCameraGroup::recomputeMapPoints,
// src/app/SL_MergeCameraGroup.cpp:1175-1183, calls per point) on map points and feature chains built with the reference's classes: the
// fixture that pins cs_recompute_map_points_keyfrms_dev.
//
// The scenes come from tests/golden/make_mergeapply_golden.py (poses, key frames, points, per point and camera 0-3 segments of
// consecutive frames with gaps and stale heads); this driver builds CamPoseItem / FeaturePoint / MapPoint objects from them the way
// ref_update_points_test.cpp's golden_relink mode does -- FeaturePoint::preFrame across a gap is what src/app/SL_CoSLAM.cpp:777-778
// assigns, FeaturePoint::bKeyFrm is "the frame is a key frame" (KeyPose marks every camera's features of a key frame) --, puts the
// points on CoSLAM::curMapPts / actMapPts / iactMapPts, asks getMapPts(fStart, fEnd) for the rows and runs the reference's function
// on them in that order.
//   ref_mergeapply_test golden <in.bin> <out.bin>          CPU only
// in.bin : int32 nScenes; per scene: int32 nCams, nFrames, frame0, nPts, fStart, fEnd, nKey; int32 keyFrames[nKey]; double sigma; per camera
//          K[9]; per camera and frame (ascending) R[9], t[3]; per point: M[3], cov[9], int32 flags (CS_MAP_* bits), firstFrame, lastFrame,
//          list (0 cur, 1 act, 2 iact); per camera int32 nSeg, per segment (newest first) int32 last, first, then (last - first + 1) x m[2]
//          newest first.
// out.bin: per scene: int32 nSelected; per point int32 selected, M[3], cov[9].
// Built by oracle/Makefile, target _ref/ref_mergeapply_test (where the reference tree exists): ref_update_points_test's link line with
// the driver swapped -- SL_CoSLAMHelper.cpp and SL_CoSLAM.cpp compiled in place with -DREF_SHIM_TRIANGULATE_ON_PATH.
// LibVisualSLAM's triangulation helpers are OUR definitions (ref_shim/ref_triangulate_impl.cpp): the vectors pin which rows are taken,
// which views, and in which order.
// TEST INFRASTRUCTURE; the binary goes to oracle/_ref/ (untracked), nothing on the GPU side needs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "app/SL_CoSLAM.h"
#include "app/SL_GlobParam.h"
#include "slam/SL_CoSLAMHelper.h"

template <class T> static bool get(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
static int geti(FILE* f) {
    int v = 0;
    if (fread(&v, 4, 1, f) != 1) {
        fprintf(stderr, "ref_mergeapply_test: short input\n");
        exit(1);
    }
    return v;
}
template <class T> static void put(FILE* f, const T* p, size_t n) { fwrite(p, sizeof(T), n, f); }
static void puti(FILE* f, int v) { fwrite(&v, 4, 1, f); }

int main(int argc, char** argv) {
    if (argc < 4 || strcmp(argv[1], "golden")) {
        fprintf(stderr, "usage: %s golden <in.bin> <out.bin>\n", argv[0]);
        return 2;
    }
    FILE* in = fopen(argv[2], "rb");
    FILE* out = fopen(argv[3], "wb");
    if (!in || !out) return 1;
    const int nScenes = geti(in);
    int nSelAll = 0, nMovedAll = 0, nPtsAll = 0;
    for (int sc = 0; sc < nScenes; ++sc) {
        const int nCams = geti(in), nFrames = geti(in), frame0 = geti(in), nPts = geti(in), fStart = geti(in), fEnd = geti(in), nKey = geti(in);
        std::set<int> keys;
        for (int k = 0; k < nKey; ++k) keys.insert(geti(in));
        double sigma;
        get(in, &sigma, 1);
        CoSLAM* co = new CoSLAM();
        co->numCams = nCams;
        std::vector<std::vector<double> > Ks(nCams, std::vector<double>(9));
        for (int c = 0; c < nCams; ++c) get(in, Ks[c].data(), 9);
        std::vector<std::vector<CamPoseItem*> > cams(nCams, std::vector<CamPoseItem*>(nFrames));
        for (int c = 0; c < nCams; ++c)
            for (int i = 0; i < nFrames; ++i) {
                cams[c][i] = new CamPoseItem();
                cams[c][i]->f = frame0 + i, cams[c][i]->camId = c;
                get(in, cams[c][i]->R, 9), get(in, cams[c][i]->t, 3);
            }
        std::vector<MapPoint*> pts(nPts);
        std::map<MapPoint*, int> indexOf;
        for (int p = 0; p < nPts; ++p) {
            double M[3];
            get(in, M, 3);
            MapPoint* mp = new MapPoint(M[0], M[1], M[2], 0);
            get(in, mp->cov, 9);
            const int flags = geti(in);
            if (flags & 2) mp->setFalse();
            else if (flags & 1) mp->setLocalDynamic();
            else mp->setLocalStatic();
            if (flags & 4) mp->setUncertain();
            mp->firstFrame = geti(in), mp->lastFrame = geti(in);
            const int list = geti(in);
            for (int c = 0; c < nCams; ++c) {
                const int nSeg = geti(in);
                FeaturePoint* newer = nullptr;
                for (int q = 0; q < nSeg; ++q) {
                    const int last = geti(in), first = geti(in);
                    for (int fr = last; fr >= first; --fr) {
                        double m[2];
                        get(in, m, 2);
                        FeaturePoint* fp = new FeaturePoint(fr, c, m[0], m[1]);
                        fp->setIntrinsic(Ks[c].data());
                        fp->setCameraPose(cams[c][fr - frame0]);
                        fp->type = TYPE_FEATPOINT_STATIC;
                        fp->bKeyFrm = keys.count(fr) != 0;
                        fp->preFrame = nullptr;
                        if (newer) newer->preFrame = fp, fp->nextFrame = newer;   // (across a gap: what SL_CoSLAM.cpp:777-778 assigns)
                        else mp->pFeatures[c] = fp;
                        newer = fp;
                    }
                }
            }
            pts[p] = mp, indexOf[mp] = p;
            if (list == 0) co->curMapPts.add(mp);
            else if (list == 1) co->actMapPts.add(mp);
            else co->iactMapPts.add(mp);
        }
        std::vector<double> before(3 * nPts);
        for (int p = 0; p < nPts; ++p) memcpy(&before[3 * p], pts[p]->M, 24);
        std::vector<MapPoint*> sel;
        co->getMapPts(fStart, fEnd, sel);                                   // SL_CoSLAM.cpp:1435
        std::vector<int> selected(nPts, 0);
        for (size_t i = 0; i < sel.size(); ++i) {
            updateStaticPointPositionAtKeyFrms(nCams, sel[i], sigma);       // SL_MergeCameraGroup.cpp:1181
            selected[indexOf[sel[i]]] = 1;
        }
        puti(out, (int)sel.size());
        for (int p = 0; p < nPts; ++p) {
            puti(out, selected[p]), put(out, pts[p]->M, 3), put(out, pts[p]->cov, 9);
            if (memcmp(&before[3 * p], pts[p]->M, 24)) ++nMovedAll;
        }
        nSelAll += (int)sel.size(), nPtsAll += nPts;
        co->curMapPts.clearWithoutRelease(), co->actMapPts.clearWithoutRelease(), co->iactMapPts.clearWithoutRelease();
    }
    fclose(in), fclose(out);
    printf("ref_mergeapply_test: %d scenes, %d points, getMapPts chose %d, %d re-triangulated\n", nScenes, nPtsAll, nSelAll, nMovedAll);
    return nMovedAll > 0 ? 0 : 1;
}
